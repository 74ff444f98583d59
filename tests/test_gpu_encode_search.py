"""-m gpu: the search stage of the LZ encoder on built inputs (tests/encode_search_cases.py; tests/test_encode_search_cpu.py shows from the reference side that each
input decides at its number and that the parse visits the proving position).  Bytes, section offsets and src_used must EQUAL the oracle's -- the helpers of the
existing encoder tests compare them -- through

  * the regular batch pipeline (test_gpu_scan_encode._regular_batch_pipeline(2): kernel B with choose_b_cap's cap of 48 / 256; no scan, no segments, no whole-GPU
    path -- each asserted),
  * the segmented path (test_gpu_mid_encode._both_ways: taken, then off, same bytes; kernel B without a cap for the flag-bit formats),
  * the whole-GPU path, one stream per call (test_gpu_big_encode._encode(expect_big=True): the one-position-per-lane kernel at every quality, cap 2 040),
  * the forced scan (mode 1; qualities 3, 8 and -- family S alone -- 9 (up to 24 candidates in one block) and, LZ4 blocks and raw Snappy, 10 (32); every stream must have gone that way).

Every case runs in two variants in the same batch: one that enc_probe_kernel gives to the two-phase kernel (enc_match_dense_kernel) and one it gives to the
one-position-per-lane kernel (enc_match_kernel with PRUNE and WAVEPOS; enc_match_dyn_kernel where matches are short or chains long).  Which kernel a stream went to
is read back (alz_debug_enc_probe_words) and held against the restated rule, stream by stream; the K6 streams stand on both sides of the line, exactly on it and one
hit below it, and on both sides of `limit` 64."""
import ctypes as C

import numpy as np
import pytest

import encode_search_cases as ES
import geometry_cases as G
import test_gpu_big_encode as BE
import test_gpu_mid_encode as ME
import test_gpu_scan_encode as SE
from gpu_common import ctx

pytestmark = pytest.mark.gpu
PAIRS = ES.PAIRS                                    # (qualities 9, 10 and raw Snappy: family S alone)
SEG_PAIRS = [(n, q) for n, q in PAIRS if G.BY_NAME[n].fmt in ME.FAMILY]
BIG_PAIRS = [(n, q) for n, q in PAIRS if G.BY_NAME[n].fmt in BE.FMTS]
SCAN_PAIRS = [(n, q) for n, q in PAIRS if n in ES.SCAN_ROWS and (q in ES.SCAN_QUALITIES or q == 10)]      # (10: ES.SCAN_Q10_ROWS, maxChain 32)
assert all(G.BY_NAME[n].fmt in SE.FAM and len(G.BY_NAME[n].props) == 1 for n in ES.SCAN_ROWS)


def _items(name, q, lanes=(False, True)):
    """[(format, raw)] and the side of each: every case of (row, quality), dense variant and lane variant"""
    row = G.BY_NAME[name]
    items, sides = [], []
    for case in ES.all_cases(name, q):
        for lane in lanes:
            items.append((row.fmt, case.buffer(lane)[0])); sides.append(lane)
    return items, sides


def _has_probe(name, q):
    """launch_match: the probe runs for the finders of the two-phase kernel with 16-bit links and one property set"""
    f = ES.finder(name, q)
    return f.max_chain >= 3 and f.max_dist <= 0xFFFF and f.props is None


def _probe_words(c, n):
    c.lib.alz_debug_enc_probe_words.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    c.lib.alz_debug_enc_probe_words.restype = C.c_int
    out = np.zeros(n, dtype=np.uint32)
    assert c.lib.alz_debug_enc_probe_words(c.h, out.ctypes.data_as(C.c_void_p), n) == n
    return out


@pytest.mark.parametrize("name,q", PAIRS)
def test_regular_batch_pipeline(name, q):
    row = G.BY_NAME[name]
    items, sides = _items(name, q)
    what = "%s search cases, regular q%d" % (name, q)
    with SE._regular_batch_pipeline(2) as c:
        seg, scan = ME._seg(c), c.lib.alz_debug_scan_streams(c.h)
        BE._encode(c, items, q, expect_big=False, what=what, **row.kw)
        assert ME._seg(c) == seg and c.lib.alz_debug_scan_streams(c.h) == scan, what
        if _has_probe(name, q):
            words = _probe_words(c, len(items))
            assert [int(w) & 1 for w in words] == [int(s) for s in sides], what


@pytest.mark.parametrize("name,q", SEG_PAIRS)
def test_segmented_path(name, q):
    row = G.BY_NAME[name]
    ME._both_ways(ctx(), _items(name, q)[0], q, "%s search cases, segmented q%d" % (name, q), **row.kw)


@pytest.mark.parametrize("name,q", BIG_PAIRS)
def test_whole_gpu_encode(name, q):
    """One stream per call; the path has no probe (launch_match without the two-phase kernel): the dense variant alone."""
    row = G.BY_NAME[name]
    for i, it in enumerate(_items(name, q, lanes=(False,))[0]):
        BE._encode(ctx(), [it], q, expect_big=True, what="%s search cases, whole-GPU q%d stream %d" % (name, q, i), **row.kw)


@pytest.mark.parametrize("name,q", SCAN_PAIRS)
def test_forced_scan(name, q):
    row = G.BY_NAME[name]
    items, _ = _items(name, q)
    with SE._regular_batch_pipeline(1) as c:
        before = c.lib.alz_debug_scan_streams(c.h)
        BE._encode(c, items, q, expect_big=False, what="%s search cases, scan q%d" % (name, q), **row.kw)
        assert c.lib.alz_debug_scan_streams(c.h) - before == len(items), (name, q)


@pytest.mark.parametrize("name,q", [("yaz0", 3), ("yaz0", 8), ("lz10", 12), ("lz10_vram", 8), ("lz4_block", 8)])
def test_probe_choice_stream_by_stream(name, q):
    """K6: 600 streams for the one-position-per-lane kernel (its list goes round the 512 rows of the grid) among 50 for the two-phase kernel, streams with `limit` 63
    and 64, and streams with exactly tot / 4 hits and one fewer: the device's word per stream is the restated rule's -- the choice and the hits per thousand."""
    row = G.BY_NAME[name]
    raws = [r for r, _ in ES.probe_batch()] + [r for r, _ in ES.probe_line()]
    want = []
    for r in raws:
        hit, tot = ES.probe_counts(name, q, r)
        want.append((int(ES.lane_side(hit, tot)) | (hit * 1000 // tot << 8)) if tot else 0)
    with SE._regular_batch_pipeline(2) as c:
        BE._encode(c, [(row.fmt, r) for r in raws], q, expect_big=False, what="%s K6 q%d" % (name, q), **row.kw)
        words = _probe_words(c, len(raws))
    assert [int(w) for w in words] == want
    assert [int(w) & 1 for w in words[-4:]] == [1, 0, 1, 0]


@pytest.mark.parametrize("name,q", ES.WORDS_PAIRS)
def test_words_choice_batches(name, q):
    """K7: 2 112 streams, half of few distinct words and half of many -- enc_words_kernel chooses per stream --, batches of 100 with either majority --
    enc_words_merge_kernel sends all one way --, and streams around 256 sampled positions: the links are the finder's whichever kernel made them, so the bytes
    are the oracle's.  (The lists are overwritten by the probe within the launch: which way a stream went is asserted through the restated rule, in the CPU file.)"""
    row = G.BY_NAME[name]
    for key, raws in sorted(ES.words_batches().items()):
        with SE._regular_batch_pipeline(2) as c:
            BE._encode(c, [(row.fmt, r) for r in raws], q, expect_big=False, what="%s K7 %s q%d" % (name, key, q), **row.kw)
