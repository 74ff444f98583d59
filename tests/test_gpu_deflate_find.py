"""-m gpu: the bytes of alz_deflate_encode_batch against tests/deflate_find_ref.py, the kernels restated in plain Python.  EXACT equality,
per case of tests/deflate_find_cases.py and per level, one batch per level (the host form, packed as tests/test_gpu_inflate.py packs, guard
bytes checked).  On a mismatch both streams are walked and the first differing block and token are reported."""
import functools

import numpy as np
import pytest

import deflate_find_cases as K
import deflate_find_ref as R
import deflate_walk as W
import test_gpu_inflate as TG
from auroralib.compression_amd import _abi as A
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def synthetic():
    return K.synthetic()


def gpu_encode(datas, level, flags):
    items = [dict(src=d, cap=R.bound(len(d))) for d in datas]
    streams, src, dst_bytes = TG.pack(items)
    dst, res = ctx().deflate_encode_batch(streams, src, dst_bytes, level, flags, dst=np.full(dst_bytes, GUARD, dtype=np.uint8))
    outs, mask = [], np.ones(dst.size, dtype=bool)
    for i, d in enumerate(datas):
        assert (res[i].status, res[i].src_used) == (A.ST_OK, len(d)), (level, flags, i)
        a = streams[i].dst_off
        outs.append(dst[a:a + res[i].dst_len].tobytes())
        mask[a:a + res[i].dst_len] = False
    assert (dst[mask] == GUARD).all(), "level %d flags %d: guard bytes overwritten" % (level, flags)
    return outs


def first_difference(got, want):
    """where two streams part: the block and the token, by walking both"""
    try:
        gb, wb = W.walk(got)[0], W.walk(want)[0]
    except ValueError as e:
        return "the GPU's stream does not walk: %s" % e
    for k, (g, w) in enumerate(zip(gb, wb)):
        if (g["type"], g["final"], g["start"], g["stored"]) != (w["type"], w["final"], w["start"], w["stored"]):
            return "block %d: GPU type %d final %d start %d, restatement type %d final %d start %d" % (k, g["type"], g["final"], g["start"], w["type"], w["final"], w["start"])
        pos = g["start"]
        for i, (a, b) in enumerate(zip(g["tokens"], w["tokens"])):
            if a != b:
                return "block %d token %d at position %d: GPU %r, restatement %r" % (k, i, pos, a, b)
            pos += 1 if a[0] == "lit" else a[1]
        if len(g["tokens"]) != len(w["tokens"]):
            return "block %d: GPU %d tokens, restatement %d" % (k, len(g["tokens"]), len(w["tokens"]))
    return "the same blocks and tokens (%d / %d blocks): the code lengths, the header or the padding differ" % (len(gb), len(wb))


def compare(cases, level, both_flags):
    datas = [c["data"] for c in cases]
    for flags in ((0, A.DEFLATE_FIXED) if both_flags else (0,)):
        outs = gpu_encode(datas, level, flags)
        for c, got in zip(cases, outs):

            def tokens_of(k, c=c):
                key = (c["name"], level, k)
                if key not in _TOKENS:
                    _TOKENS[key] = R.find(c["data"], k, level)
                return _TOKENS[key]
            want = b"".join(b["bytes"] for b in R.blocks(c["data"], level, flags, tokens_of=tokens_of))
            assert got == want, "%s, level %d, flags %d: %d bytes against %d: %s" % (c["name"], level, flags, len(got), len(want), first_difference(got, want))


_TOKENS = {}                   # the restatement's find runs once per (case, level, block), whatever the flags


@pytest.mark.parametrize("level", range(10))
def test_synthetic_cases_equal_the_restatement(level):
    compare(synthetic(), level, both_flags=level in (0, 6))


@pytest.mark.parametrize("level", range(10))
def test_bmp_and_text_equal_the_restatement(test_bmp, level):
    compare(K.corpus(test_bmp), level, both_flags=True)
