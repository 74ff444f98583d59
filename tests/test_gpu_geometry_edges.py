"""-m gpu: every format's distance and length limits on every encoder and decoder path.  The inputs are those of tests/geometry_cases.py -- repeats planted at
max_dist - 1, max_dist and max_dist + 1, at both sides of every tier and token-form step, of exactly min_len and max_len, periodic runs that end k bytes
past max_len, literal runs at both sides of every count step, and the same plants behind 0..7 / 0..63 leading bytes (every flag-bit position, every lane of the
64-position window walk).  tests/test_geometry_edges_cpu.py shows, from the reference side alone, that these inputs reach the limits.

Encoder: bytes, section offsets and src_used IDENTICAL to the oracle's at qualities 0 (the fused search), 8 and 12 (the min-length table, a capped cursor), through
  * the regular batch pipeline (test_gpu_scan_encode._regular_batch_pipeline(2): no scan, no segments, no whole-GPU path -- each asserted),
  * the forced scan path (mode 1; its formats, flag-bit windows up to 8 KiB -- every stream must have gone that way),
  * the segmented path (test_gpu_mid_encode._both_ways: taken, then off, same bytes),
  * the whole-GPU path (test_gpu_big_encode._encode(expect_big=True); a format of the path whose geometry it does not take -- links beyond 16 bits -- must NOT take it),
and every body decodes back on the GPU (where the reference's own reader reads it back: geometry_cases.Row.decodable).

Decoder: the oracle's quality-8 bodies of the same inputs, and hand-assembled streams for what no encoder writes at the limit (a token at distance W with fewer
than W bytes produced, distance W at the last output byte, max_len ending exactly at decom_len and one byte beyond), through the default kernels and the exact
ones (gpu_common.compare_batch), kernel variants 1 and 2 into canary-filled destinations (test_gpu_canary.canary_decode), alz_measure_batch
(test_gpu_measure.measure_parity) and the whole-GPU path (test_gpu_big_stream._one, taken for streams of its formats; the hand-assembled streams of 24 KiB and more
go through it too).  Hand-assembled streams exist for all 25 bodies (EDGE_FORMATS); where a grammar has no such stream the case is left out with the C# line beside it."""
import functools

import numpy as np
import pytest

import geometry_cases as G
import oracle_lib as O
import test_gpu_big_encode as BE
import test_gpu_big_stream as BS
import test_gpu_mid_encode as ME
import test_gpu_scalar_paths as SP
import test_gpu_scan_encode as SE
import token_bodies as TB
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import synth
from gpu_common import compare_batch, ctx, pack_streams
from test_gpu_canary import canary_decode
from test_gpu_measure import measure_parity

pytestmark = pytest.mark.gpu
QUALITIES = (0, 8, 12)
ROW_IDS = [r.name for r in G.ROWS]
SEQ = (A.FMT_LZ4_BLOCK, A.FMT_SNAPPY_RAW)
SCAN_ROWS = [r.name for r in G.ROWS if r.fmt in SE.FAM and len(r.props) == 1 and (r.fmt in SEQ or r.max_dist <= 8192)]
SEG_ROWS = [r.name for r in G.ROWS if r.fmt in ME.FAMILY]
BIG_ROWS = [r.name for r in G.ROWS if r.fmt in BE.FMTS]


def _raws(row, phases=True):
    return [G.planted(row)[0]] + (G.phases(row) if phases else [])


def _items(row, phases=True):
    return [(row.fmt, r) for r in _raws(row, phases)]


@functools.lru_cache(maxsize=None)
def _oracle_bodies(name, quality):
    row = G.BY_NAME[name]
    out = []
    for raw in _raws(row):
        body, aux = O.encode_stream(row.fmt, raw, quality=quality, **row.kw)
        out.append((body, aux.aux0, aux.aux1))
    return out


def _decode_items(row, raws, bodies):
    sized = row.fmt not in BS.ELEM
    return [dict(fmt=row.fmt, src=b, decom_len=len(r) if sized else 0, cap=len(r), aux0=a0, aux1=a1) for r, (b, a0, a1) in zip(raws, bodies)]


def _decode_back(row, raws, bodies, quality, what):
    """compare_batch: the GPU against the oracle on both kernel families; and the bytes are the input's where the reference reads its own body back."""
    streams, src, dst_bytes = pack_streams(_decode_items(row, raws, bodies))
    gr, g_dst = compare_batch(streams, src, dst_bytes, lz=row.kw.get("lz"), what=what)
    if row.decodable and quality >= row.decodable_from:
        rec = synth.stream_records(streams)
        for i, r in enumerate(raws):
            a = int(rec["dst_off"][i])
            assert gr["status"][i] == A.ST_OK and bytes(g_dst[a:a + len(r)]) == r, (what, i)


# ------------------------------------------------------------------------------------------------ encoder
@pytest.mark.parametrize("name", ROW_IDS)
def test_regular_batch_pipeline(name):
    row = G.BY_NAME[name]
    items = _items(row)
    for q in QUALITIES:
        what = "%s regular q%d" % (name, q)
        with SE._regular_batch_pipeline(2) as c:
            seg, scan = ME._seg(c), c.lib.alz_debug_scan_streams(c.h)
            got = BE._encode(c, items, q, expect_big=False, what=what, **row.kw)
            assert ME._seg(c) == seg and c.lib.alz_debug_scan_streams(c.h) == scan, what
        assert got == [b for b, _, _ in _oracle_bodies(name, q)]
        _decode_back(row, [r for _, r in items], _oracle_bodies(name, q), q, what)


@pytest.mark.parametrize("name", SCAN_ROWS)
def test_forced_scan(name):
    row = G.BY_NAME[name]
    items = _items(row)
    for q in (3, 8):                                      # (the path covers qualities 2..9: max_chain 3..32)
        with SE._regular_batch_pipeline(1) as c:
            before = c.lib.alz_debug_scan_streams(c.h)
            BE._encode(c, items, q, expect_big=False, what="%s scan q%d" % (name, q), **row.kw)
            assert c.lib.alz_debug_scan_streams(c.h) - before == len(items), (name, q)


@pytest.mark.parametrize("name", [r.name for r in G.ROWS if r.fmt in SE.FAM and r.name not in SCAN_ROWS])
def test_forced_scan_leaves_wider_flag_bit_windows_alone(name):
    """A flag-bit format whose window is wider than 8 KiB -- LZSS with 14, 15 and 16 window bits -- does not scan even when forced."""
    row = G.BY_NAME[name]
    with SE._regular_batch_pipeline(1) as c:
        before = c.lib.alz_debug_scan_streams(c.h)
        BE._encode(c, _items(row), 8, expect_big=False, what=name + " forced scan, not eligible", **row.kw)
        assert c.lib.alz_debug_scan_streams(c.h) == before, name


@pytest.mark.parametrize("name", SEG_ROWS)
def test_segmented_path(name):
    row = G.BY_NAME[name]
    items = _items(row)
    for q in QUALITIES:
        ME._both_ways(ctx(), items, q, "%s segmented q%d" % (name, q), **row.kw)


@pytest.mark.parametrize("name", BIG_ROWS)
def test_whole_gpu_encode(name):
    """One stream per call.  The path links positions with 16-bit distances: a geometry whose window is wider (LZSS with 16 window bits: 65536) stays off it."""
    row = G.BY_NAME[name]
    for q in QUALITIES:
        for i, r in enumerate(_raws(row)):
            BE._encode(ctx(), [(row.fmt, r)], q, expect_big=row.max_dist <= 0xFFFF, what="%s whole-GPU q%d stream %d" % (name, q, i), **row.kw)


# ------------------------------------------------------------------------------------------------ decoder
@pytest.mark.parametrize("name", ROW_IDS)
def test_decode_the_oracles_bodies_on_every_path(name):
    row = G.BY_NAME[name]
    raws, bodies, lz = _raws(row), _oracle_bodies(name, 8), row.kw.get("lz")
    _decode_back(row, raws, bodies, 8, name + " decode")
    streams, src, dst_bytes = pack_streams(_decode_items(row, raws, bodies), dst_slack=16)
    canary_decode(streams, src, dst_bytes, lz=lz, what=name + " decode", variants=(0, 1, 2))
    measure_parity(streams, src, dst_bytes, lz=lz, what=name + " measure")
    for i, (r, (body, a0, a1)) in enumerate(zip(raws, bodies)):
        assert len(r) >= 24 << 10
        BS._one(ctx(), row.fmt, body, len(r), a0, a1, expect_big=row.fmt in BS.FMTS, what="%s whole-GPU decode, stream %d" % (name, i), lz=lz)


# ---- hand-assembled streams: what no encoder of ours writes at the limit (the writers: tests/token_bodies.py)
LIT, MATCH = SP.LIT, SP.MATCH
EDGE_FORMATS, FIRST_IS_LITERAL = TB.EDGE_FORMATS, TB.FIRST_IS_LITERAL


def _edge_token_lists(W, min_len, max_len, rng):
    """(name, tokens, declared size relative to what the tokens give)"""
    lit = lambda k: [(LIT, int(x)) for x in rng.integers(1, 256, k)]       # noqa: E731
    n = min(max_len, 1028)
    out = [("distance W after 5 bytes", lit(5) + [(MATCH, W, min(n, 10))] + lit(3), 0),
           ("distance W as the first token", [(MATCH, W, min_len)] + lit(9), 0),
           ("distance W at the last byte", lit(W) + [(MATCH, 3, n)] + lit(2) + [(MATCH, W, min_len)], 0),
           ("distance W - 1 and W after W bytes", lit(W) + [(MATCH, W, min_len + 1), (MATCH, W - 1, min_len)] + lit(1), 0),
           ("max_len ends at decom_len", lit(7) + [(MATCH, 7, n)], 0),
           ("max_len ends one byte beyond decom_len", lit(7) + [(MATCH, 7, n)], -1),
           ("max_len from before the start", lit(2) + [(MATCH, W, n)] + lit(2), 0),
           ("distance W at the last byte of 24 KiB", lit(24 << 10) + [(MATCH, W, min_len)], 0)]      # (long enough for the whole-GPU path)
    return out


def _edge_items(name):
    fmt, W, min_len, max_len, body, lz = EDGE_FORMATS[name]
    rng = np.random.default_rng(8800 + fmt)
    items = []
    for what, toks, delta in _edge_token_lists(W, min_len, max_len, rng):
        if fmt == A.FMT_LZ4_BLOCK:
            toks = toks + [(LIT, 7)] * 5                 # (a block ends in literals)
        if fmt in FIRST_IS_LITERAL and toks[0][0] == MATCH:
            continue
        raw = SP.expand(toks)
        it = SP.assemble(fmt, toks, lz) if body is None else body(toks)
        if not isinstance(it, dict):
            it = dict(fmt=fmt, src=it)
        # BLZ alone refuses a source before the stream start (destination[dst - 1 + distance] throws, BLZ.cs:121-126): those streams are compared with the oracle's
        # status, not with the expansion
        pos, early = 0, False
        for t in toks:
            early = early or (t[0] == MATCH and t[1] > pos)
            pos += 1 if t[0] == LIT else t[2]
        exact = delta == 0 and not (fmt == A.FMT_BLZ and early)
        sized = fmt not in BS.ELEM
        it.update(decom_len=(len(raw) + delta) if sized else 0, cap=len(raw) + delta, want=raw if exact else None, cut=not exact, what=what)
        items.append(it)
    return items, lz


@pytest.mark.parametrize("name", sorted(EDGE_FORMATS))
def test_hand_assembled_tokens_at_the_limits(name):
    items, lz = _edge_items(name)
    fmt = items[0]["fmt"]
    SP.run(items, name + " limits", lz=lz)
    streams, src, dst_bytes = pack_streams(items, dst_slack=16)
    measure_parity(streams, src, dst_bytes, lz=lz, what=name + " limits, measured")
    big = [it for it in items if it["want"] is not None and len(it["want"]) >= 24 << 10]
    assert big
    for it in big:                                       # one by one: the whole-GPU path, taken by the formats that have it
        BS._one(ctx(), fmt, it["src"], len(it["want"]), it.get("aux0", 0), it.get("aux1", 0), expect_big=fmt in BS.FMTS, what="%s limits, whole-GPU: %s" % (name, it["what"]), lz=lz)
