"""Writes tests/golden/geometry_clamp.json: for every row of tests/geometry_cases.py with a finite max_len, what the finder restatement
(tests/chain_finder_ref.py, quality 8) does on periodic runs whose available match length is max_len + k -- the clamped match and what it leaves
behind.  tests/test_geometry_edges_cpu.py compares the finder with this file and pins the finder to the oracle on the same streams, so a change of
either shows up.  Run from the repository root: python tests/golden/make_geometry_clamp.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import geometry_cases as G                      # noqa: E402
import test_geometry_edges_cpu as T             # noqa: E402

if __name__ == "__main__":
    out = {r.name: T.clamp_record(r.name) for r in G.ROWS}
    out = {k: v for k, v in out.items() if v}
    with open(os.path.join(HERE, "geometry_clamp.json"), "w") as fh:
        fh.write("{\n" + ",\n".join(' "%s": %s' % (k, json.dumps(out[k], separators=(",", ":"), sort_keys=True)) for k in sorted(out)) + "\n}\n")
