"""Writes tests/golden/deflate_find_vectors.json: the length and the SHA-256 of tests/deflate_find_ref.py's encode() per (case, level, flags)
over every case of tests/deflate_find_cases.py (deflate_find_cases.vectors, which tests/test_deflate_find_cpu.py calls as well to regenerate
and compare), so an edit of the restatement cannot drift unseen; run this only after the GPU has confirmed the new bytes
(tests/test_gpu_deflate_find.py).
    python tests/golden/make_deflate_find_vectors.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import deflate_find_cases as K  # noqa: E402


def main():
    vectors = K.vectors(K.synthetic() + K.corpus(K.load_test_bmp()))
    with open(os.path.join(HERE, "deflate_find_vectors.json"), "w") as f:
        json.dump({"key": "case|level|flags -> [bytes, sha256]", "vectors": vectors}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(vectors), "vectors")


if __name__ == "__main__":
    main()
