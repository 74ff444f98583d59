#!/usr/bin/env python3
"""Generates tests/golden/ref_surfaces.json: the public surface of every reference class a shim class replaces -- its interface
list, its public settable properties with type and default, and its static body entry points with return and parameter types
(names and default arguments included) -- read by the same extraction tests/test_shim_binding.py applies to the shim.  Names and
signatures only, no code.  tests/test_shim_binding.py compares the shim against this file, so the check needs no reference tree.

Run from the repository root with the reference's source directory (the one holding AuroraLib.Compression/):
    python tests/golden/make_ref_surfaces.py REF_SRC"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_shim_binding import REF_CLASSES, REF_SURFACES, _surface  # noqa: E402


def main(ref_src):
    out = {}
    for key, (cls, files) in sorted(REF_CLASSES.items()):
        ifaces, props, statics = set(), {}, {}
        for f in files:
            i, p, st = _surface(open(os.path.join(ref_src, f), encoding="utf-8-sig").read(), cls)
            ifaces |= i
            props.update(p)
            for k, v in st.items():
                statics.setdefault(k, set()).update(v)
        out[key] = {"class": cls, "files": files, "interfaces": sorted(ifaces), "properties": {k: list(v) for k, v in sorted(props.items())},
                    "statics": {k: sorted([ret, list(params)] for ret, params in v) for k, v in sorted(statics.items())}}
    with open(REF_SURFACES, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
