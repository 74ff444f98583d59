"""-m gpu: the refusals of the entry points of csrc/alz_host.cpp, replayed: every call of tests/golden/make_host_refusals.py (NULL arguments, unknown
kinds, ranges outside the stated sizes, geometries and settings the GPU path does not take, unusable context lists, two refusals in one batch in
both orders, the empty batches) must give the return code and the alz_last_error() text recorded in tests/golden/host_refusals.json, byte for byte.
No kernel runs: every call is refused before a launch, or is an empty batch.  It needs a context, hence a device."""
import importlib.util
import json
import os

import pytest

from gpu_common import ctx

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_host_refusals", os.path.join(GOLDEN, "make_host_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_refusals_are_the_recorded_ones():
    want = json.load(open(os.path.join(GOLDEN, "host_refusals.json")))["cases"]
    c = ctx()
    got = _generator().run_table(c.lib, c.h)
    assert [g[0] for g in got] == [w[0] for w in want], "the table of calls and the recorded file differ: regenerate on the commit whose answers are pinned"
    bad = [(g, w) for g, w in zip(got, want) if list(g) != list(w)]
    assert not bad, "%d of %d answers differ; the first: got %r, recorded %r" % (len(bad), len(want), bad[0][0], bad[0][1])
    assert sum(1 for w in want if w[1] != 0) > 300 and sum(1 for w in want if w[1] == 0) >= 30    # the refusals, and the empty batch of every entry point
