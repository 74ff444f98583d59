"""usage: python tests/golden/make_apenc_kats.py  -- writes tests/golden/apenc_far.json: the known answers of the aPLib encoder tests whose expected body
takes long to compute in pure Python (inputs above 256 KiB).  Per case: the generator's parameters, the input's length and SHA-256, the body's length
and SHA-256 as the restatement (tests/apenc_ref.py over tests/chain_finder_ref.py) gives them, and the far matches it took.  tests/test_apenc_cpu.py
regenerates and compares (about 20 s of CPU time for the 2 MiB case); tests/test_gpu_apenc.py builds the input from the parameters and only hashes.

A case is `filler` bytes in which no four bytes repeat, then `plants`: per (distance, length) the `length` bytes found `distance` back, copied to the
end, and a separator that occurs nowhere else -- a repeat the finder can take at exactly that distance, or must leave alone."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

CASES = {
    # the last two property sets: (0x100000, max, 7) and (0x200000, max, 8).  Taken: 7 bytes at 0x100000, 8 at 0x100001 (the last set's minimum), 8 at
    # 0x1FFFFF and at exactly 0x200000; left alone: 6 at 0x100000, 7 at 0x100001 and at 0x200000, anything at 0x200001
    "far": {"filler": 0x200000 + 16, "quality": 8, "strategy": 0,
            "plants": [[0x100000, 6], [0x100000, 7], [0x100001, 7], [0x100001, 8], [0x1FFFFF, 8], [0x200000, 7], [0x200000, 8], [0x200001, 8], [0x200001, 40]]},
}


def filler(n):
    """n bytes, all 0x80 and above, in which no group of four repeats wherever it starts: a 20-bit counter, five bits per byte, the byte's place in bits 5-6"""
    c = np.arange((n + 3) // 4, dtype=np.uint32)
    out = np.empty((len(c), 4), dtype=np.uint8)
    for k in range(4):
        out[:, k] = 0x80 | (k << 5) | ((c >> (5 * k)) & 0x1F)
    return out.reshape(-1)[:n].tobytes()


def build(case):
    data = bytearray(filler(case["filler"]))
    for k, (dist, length) in enumerate(case["plants"]):
        p = len(data)
        data += data[p - dist:p - dist + length]
        data += bytes([1 + k, 0x21 + k, 0x41 + k, 0x61 + k, 1 + k])            # (below 0x80: in no group of four of the filler, and in no other separator)
    return bytes(data)


def answer(case):
    import apenc_ref as E
    data = build(case)
    trace = []
    body = E.compress_headerless(data, case["quality"], case["strategy"], None, trace)
    far = sorted([d, ln] for kind, _, _, d, ln in trace if kind in ("match", "match_biased", "rep") and d >= 0x100000)
    return {"params": case, "input_len": len(data), "input_sha256": hashlib.sha256(data).hexdigest(),
            "body_len": len(body), "body_sha256": hashlib.sha256(body).hexdigest(), "far_matches": far}


if __name__ == "__main__":
    out = {name: answer(case) for name, case in CASES.items()}
    with open(os.path.join(HERE, "apenc_far.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: (v["body_len"], v["far_matches"]) for k, v in out.items()}))
