"""Writes tests/golden/encode_search_digests.json: the number of cases and a digest of their buffers and claims for every (row, quality, family) of
tests/encode_search_cases.py, and of the K6 streams.  tests/test_encode_search_cpu.py compares the builders with this file, so a change of a builder is
noticed.  Run from the repository root: python tests/golden/make_encode_search_digests.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_encode_search_cpu as T              # noqa: E402

if __name__ == "__main__":
    with open(os.path.join(HERE, "encode_search_digests.json"), "w") as fh:
        json.dump(T.digests(), fh, indent=1, sort_keys=True)
        fh.write("\n")
