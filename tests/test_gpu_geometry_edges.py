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


# ---- hand-assembled streams: what no encoder of ours writes at the limit
LIT, MATCH = SP.LIT, SP.MATCH


def _lz40_body(tokens):                                  # LZ40.cs:72-118: flag bits MSB first, negated; u16 LE distance << 4 | length
    body = bytearray()
    for i in range(0, len(tokens), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 8]):
            if t[0] == LIT:
                data.append(t[1])
                continue
            fb |= 0x80 >> k
            _, d, n = t
            if n < 16:
                data += ((d << 4) | n).to_bytes(2, "little")
            elif n < 272:
                data += (d << 4).to_bytes(2, "little") + bytes([n - 16])
            else:
                data += ((d << 4) | 1).to_bytes(2, "little") + (n - 272).to_bytes(2, "little")
        body.append((-fb) & 0xFF)
        body += data
    return bytes(body)


def _flag8_body(tokens, match_bytes, msb=True):
    body = bytearray()
    for i in range(0, len(tokens), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 8]):
            if t[0] == LIT:
                data.append(t[1])
            else:
                fb |= (0x80 >> k) if msb else (1 << k)
                data += match_bytes(t[1], t[2])
        body.append(fb)
        body += data
    return bytes(body)


def _clz0(d, n):                                         # CLZ0.cs:99-130
    delta = 0x1000 - d
    return bytes([delta & 0xFF, (n - 3) | ((delta >> 8) << 4)])


def _seq_body(fmt, tokens):
    """LZ4 blocks (LZ4.cs:202-238), raw Snappy (Snappy.cs:124-203) and CNS (CNS.cs:111-141) from a token list"""
    out, lits = bytearray(), bytearray()
    total = len(SP.expand(tokens))
    if fmt == A.FMT_SNAPPY_RAW:
        v = total
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80); v >>= 7
        out.append(v)

    def ext(v):
        v -= 15
        b = bytearray()
        if v >= 0:
            while True:
                x = min(v, 255); b.append(x); v -= x
                if x != 255:
                    return b
        return b

    def flush_lits():
        if fmt == A.FMT_SNAPPY_RAW and lits:
            n = len(lits)
            out.extend(bytes([(n - 1) << 2]) if n <= 60 else bytes([60 << 2, n - 1]) if n <= 256 else bytes([61 << 2]) + (n - 1).to_bytes(2, "little"))
            out.extend(lits)
        if fmt == A.FMT_CNS:
            for i in range(0, len(lits), 127):
                out.append(len(lits[i:i + 127])); out.extend(lits[i:i + 127])
        del lits[:]
    for t in tokens + [None]:
        if t is not None and t[0] == LIT:
            lits.append(t[1])
            continue
        if fmt == A.FMT_LZ4_BLOCK:
            n = t[2] - 4 if t else 0
            out.append((min(len(lits), 15) << 4) | min(n, 15))
            out += ext(len(lits)) + lits
            del lits[:]
            if t:
                out += t[1].to_bytes(2, "little") + ext(n)
            continue
        flush_lits()
        if t is None:
            break
        _, d, n = t
        if fmt == A.FMT_SNAPPY_RAW:
            out += bytes([2 | ((n - 1) << 2)]) + d.to_bytes(2, "little")
        else:
            out += bytes([0x80 | (n - 3), d - 1])
    return bytes(out)


def _lz02(d, n):                                         # LZ02.cs:133-146
    return bytes([((d >> 8) << 4) | (n - 1 if n <= 16 else 0), d & 0xFF]) + (bytes([n - 17]) if n > 16 else b"")


def _lz02_body(tokens):
    """the tokens, then the terminator: a match token of distance 0  LZ02.cs:147-149"""
    body = bytearray()
    toks = tokens + [None]
    for i in range(0, len(toks), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(toks[i:i + 8]):
            if t is not None and t[0] == LIT:
                data.append(t[1])
            else:
                fb |= 0x80 >> k
                data += bytes(2) if t is None else _lz02(t[1], t[2])
        body.append(fb)
        body += data
    return bytes(body)


def _runs(tokens):
    """[(literals in front, match or None)]"""
    out, lits = [], bytearray()
    for t in tokens:
        if t[0] == LIT:
            lits.append(t[1])
        else:
            out.append((bytes(lits), t)); lits = bytearray()
    out.append((bytes(lits), None))
    return out


def _wflz_body(tokens, big):
    """WFLZ.cs:161-196: blocks of distance (u16), length - 4, literal count, literals; a block without a match carries literals only; four zero bytes end the stream"""
    out = bytearray()
    pending = (0, 0)
    for lits, m in _runs(tokens):
        first = True
        while first or lits:
            d, n = pending
            out += d.to_bytes(2, "big" if big else "little") + bytes([n - 4 if n else 0, min(len(lits), 255)]) + lits[:255]
            lits, pending, first = lits[255:], (0, 0), False
        if m is not None:
            pending = (m[1], m[2])
    if pending != (0, 0):
        out += pending[0].to_bytes(2, "big" if big else "little") + bytes([pending[1] - 4, 0])
    return bytes(out + bytes(4))


def _refpack_body(tokens):
    """RefPack.cs:241-303 through the writer that pins the finder restatement (tests/test_bitenc_cpu.py: refpack_write): the canonical form of every token"""
    from test_bitenc_cpu import refpack_write
    raw, ms, pos = SP.expand(tokens), [], 0
    for t in tokens:
        if t[0] == MATCH:
            ms.append((pos, t[1], t[2]))
        pos += 1 if t[0] == LIT else t[2]
    return refpack_write(raw, ms + [(len(raw), 0, 0)])


def _yay0_token(d, n, extra):                            # Yay0.cs:165-177: lengths from 18 on put a byte into the literal stream
    if n < 18:
        return (((n - 2) << 12) | (d - 1)).to_bytes(2, "big")
    extra.append(n - 0x12)
    return (d - 1).to_bytes(2, "big")


def _lzhudson_body(tokens):
    """Yaz0's tokens under flag words of 32 bits, big-endian, first token in the top bit, 1 = literal  LZHudson.cs:55-59"""
    body = bytearray()
    for i in range(0, len(tokens), 32):
        fw, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 32]):
            if t[0] == LIT:
                fw |= 0x80000000 >> k
                data.append(t[1])
            else:
                extra = []
                data += _yay0_token(t[1], t[2], extra) + bytes(extra)
        body += fw.to_bytes(4, "big") + data
    return bytes(body)


def _smsr00_item(tokens):
    """SMSR00.cs:85-131: a section of 16-bit big-endian words -- a mask (first token in the top bit, 1 = literal), then the match words of its 16 tokens -- and the
    literals behind it; aux0 = the length of the first section"""
    codes, lits = bytearray(), bytearray()
    for i in range(0, len(tokens), 16):
        mask, words = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 16]):
            if t[0] == LIT:
                mask |= 0x8000 >> k
                lits.append(t[1])
            else:
                words += (((t[2] - 3) << 12) | (t[1] - 1)).to_bytes(2, "big")
        codes += mask.to_bytes(2, "big") + words
    return dict(fmt=A.FMT_SMSR00, src=bytes(codes + lits), aux0=len(codes), aux1=0)


def _prs_body(tokens, big):
    """PRS.cs:104-159 with the reference's FlagWriter (tests/chain_finder_ref.py): short form for lengths 2..5 at distances up to 0x100, else the long form"""
    from chain_finder_ref import FlagWriter
    fw = FlagWriter(big)
    order = "big" if big else "little"
    for t in tokens:
        if t[0] == LIT:
            fw.buffer.append(t[1]); fw.write_bit(1)
            continue
        _, d, n = t
        fw.write_bit(0)
        if d <= 0x100 and n <= 5:
            fw.write_bit(0); fw.write_bit(((n - 2) >> 1) & 1); fw.write_bit((n - 2) & 1)
            fw.buffer.append((-d) & 0xFF)
            fw.flush_if_necessary()
        else:
            v = ((-d) << 3) & 0xFFFF
            fw.buffer += (v | (n - 2 if n <= 9 else 0)).to_bytes(2, order) + (bytes([n - 1]) if n > 9 else b"")
            fw.write_bit(1)
    fw.write_bit(0); fw.buffer += bytes(2); fw.write_bit(1)
    fw.flush()
    return bytes(fw.out)


def _cnx2_body(tokens):
    """CNX2.cs:140-172: two flag bits per element, least significant first: 01 one literal, 11 a counted run, 10 a match"""
    from chain_finder_ref import FlagWriter
    fw = FlagWriter(False)
    for lits, m in _runs(tokens):
        while lits:
            c = lits[:255]
            if len(c) == 1:
                fw.buffer.append(c[0]); fw.write_bit(1); fw.write_bit(0)
            else:
                fw.buffer.append(len(c)); fw.buffer += c; fw.write_bit(1); fw.write_bit(1)
            lits = lits[255:]
        if m is not None:
            fw.buffer += ((((m[1] - 1) & 0x7FF) << 5) | ((m[2] - 4) & 0x1F)).to_bytes(2, "big")
            fw.write_bit(0); fw.write_bit(1)
    fw.flush()
    return bytes(fw.out)


def _blz_token(d, n):                                    # BLZ.cs:97-135 in stream order: distance - 3 in twelve bits
    return (((n - 3) << 12) | (d - 3)).to_bytes(2, "big")


def _fastlz_body(tokens, level2):
    """FastLZ.cs:162-245: literal runs of at most 32; the level rides on the first byte, which is a literal run's"""
    out, first = bytearray(), level2
    for lits, m in _runs(tokens):
        while lits:
            c = lits[:32]
            out.append((len(c) - 1) | (0x20 if first else 0)); out += c
            first, lits = False, lits[32:]
        if m is None:
            continue
        length, distance = m[2] - 3, m[1] - 1
        short = min(distance, 0x1FFF) if level2 else distance
        out.append(((min(length, 6) + 1) << 5) | (short >> 8))
        if length >= 6:
            length -= 6
            while level2 and length >= 255:
                out.append(255); length -= 255
            out.append(length)
        out.append(short & 0xFF)
        if level2 and distance >= 0x1FFF:
            out += (distance - 0x1FFF).to_bytes(2, "big")
    return bytes(out)


def _shrek_field(v, at):
    return (v, b"") if v < at else (0x1E, bytes([v - at])) if v < at + 256 else (0x1F, (v - at - 256).to_bytes(2, "little"))


def _lzshrek_body(tokens):
    """LZShrek.cs:121-174: a group = literal count field << 3 | matches - 1, the literals, up to eight matches; four zero bytes end the stream"""
    out = bytearray()
    runs = _runs(tokens)
    i = 0
    while i < len(runs):
        lits, m = runs[i]
        group = bytearray()
        count = 0
        while m is not None:
            _, d, n = m
            df, dx = _shrek_field(d - 1, 30)
            group += bytes([(df << 3) | (n if n <= 7 else 0)]) + (bytes([n - 7]) if n > 7 else b"") + dx
            count += 1
            if count == 8 or i + 1 >= len(runs) or runs[i + 1][0] or runs[i + 1][1] is None:
                break
            i += 1
            m = runs[i][1]
        i += 1
        if m is None and not lits:
            break
        uf, ux = _shrek_field(len(lits), 30)
        out += bytes([(uf << 3) | max(count - 1, 0)]) + ux + lits + group
    return bytes(out + bytes(4))


def _hig_raw(lits):                                      # HIG.cs:234-243: count - 2 in a byte (3..257), else 0 and the count as a ushort
    return (bytes([len(lits) - 2]) if 3 <= len(lits) <= 257 else bytes([0]) + len(lits).to_bytes(2, "little")) + lits


def _hig_body(tokens):
    """HIG.cs:214-323: an initial literal block, then matches whose two low bits say what follows: 3 nothing, 1 / 2 that many literals, 0 a literal block"""
    runs = _runs(tokens)
    out = bytearray(_hig_raw(runs[0][0]))
    for k, (_, m) in enumerate(runs):
        if m is None:
            break
        _, d, n = m
        follow = runs[k + 1][0]
        code = 3 if not follow else len(follow) if len(follow) < 3 else 0
        if d <= 0x7FF and n <= 9:
            out.append(code | ((n - 4) << 5) | ((d >> 6) & 0x1C))
        else:
            if d <= 0x3FFF and n <= 35:
                out.append(0xC0 | (n - 4))
            else:
                out.append(0xE0 | ((d >> 10) & 0x10) | (n - 3 if n <= 18 else 0))
                if n > 18:
                    out += bytes([n - 18]) if n <= 273 else bytes([0]) + n.to_bytes(2, "big")
            out.append(code | ((d >> 6) & 0xFC))
        out.append(d & 0xFF)
        out += _hig_raw(follow) if code == 0 else follow
    return bytes(out)


def _lzo_ext(v):                                         # LZO.cs:263-271
    out = bytearray()
    while v > 255:
        out.append(0); v -= 255
    return bytes(out + bytes([v]))


def _lzo_body(tokens):
    """LZO.cs:49-139 read backwards: literal runs of 1..3 ride in the two low bits of the match in front (or, at the start, in a first byte of 17 + count), longer runs
    have an instruction of their own; M2 for lengths up to 8 at distances up to 2048, M3 up to 16384, M4 beyond; 11 00 00 ends the stream"""
    runs = _runs(tokens)
    out = bytearray()
    first = runs[0][0]
    if 0 < len(first) <= 238:
        out += bytes([17 + len(first)]) + first
    for k, (lits, m) in enumerate(runs):
        if k and len(lits) > 3 or not k and len(lits) > 238:
            out += (bytes([len(lits) - 3]) if len(lits) <= 18 else bytes([0]) + _lzo_ext(len(lits) - 18)) + lits
        if m is None:
            break
        _, d, n = m
        follow = runs[k + 1][0]
        p = len(follow) if len(follow) <= 3 else 0
        if n <= 8 and d <= 2048:
            out.append(p | (((d - 1) & 7) << 2) | ((0x40 | ((n - 3) << 5)) if n <= 4 else (0x80 | ((n - 5) << 5))))
            out.append((d - 1) >> 3)
        elif d <= 16384:
            out += bytes([0x20 | (n - 2)]) if n <= 33 else bytes([0x20]) + _lzo_ext(n - 33)
            out += bytes([p | (((d - 1) << 2) & 0xFF), (d - 1) >> 6])
        else:
            dd = d - 0x4000
            flag = 0x10 | ((dd & 0x4000) >> 11)
            out += bytes([flag | (n - 2)]) if n <= 9 else bytes([flag]) + _lzo_ext(n - 9)
            out += bytes([p | ((dd << 2) & 0xFF), (dd >> 6) & 0xFF])
        if p:
            out += follow
    return bytes(out + b"\x11\x00\x00")


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


EDGE_FORMATS = {
    # name: (format, window, min_len, max_len, body(tokens) -> bytes or None for test_gpu_scalar_paths.assemble, lz)
    "lzss_12_4_2": (A.FMT_LZSS, 0x1000, 3, 18, None, A.LzProperties.from_bits(12, 4, 2)),
    "lzss_10_6_2": (A.FMT_LZSS, 0x400, 3, 66, None, A.LzProperties.from_bits(10, 6, 2)),      # (distance and length bits fill the token's 16: wider geometries have no body to assemble)
    "lzss_8_4_2": (A.FMT_LZSS, 0x100, 3, 18, None, A.LzProperties.from_bits(8, 4, 2)),
    "lz10": (A.FMT_LZ10, 0x1000, 3, 18, None, None),
    "lz11": (A.FMT_LZ11, 0x1000, 3, 0x4000, None, None),
    "yaz0": (A.FMT_YAZ0, 0x1000, 3, 273, None, None),
    "yay0": (A.FMT_YAY0, 0x1000, 3, 273, None, None),
    "mio0": (A.FMT_MIO0, 0x1000, 3, 18, None, None),
    "lz40": (A.FMT_LZ40, 0xFFF, 3, 0x4000, _lz40_body, None),                 # (12 distance bits, no bias: 0xFFF is the farthest a token can say)
    "clz0": (A.FMT_CLZ0, 0x1000, 3, 18, lambda t: _flag8_body(t, _clz0, msb=False), None),
    "lz4_block": (A.FMT_LZ4_BLOCK, 0xFFFF, 4, 100000, lambda t: _seq_body(A.FMT_LZ4_BLOCK, t), None),
    "snappy_raw": (A.FMT_SNAPPY_RAW, 0x8000, 4, 64, lambda t: _seq_body(A.FMT_SNAPPY_RAW, t), None),
    "cns": (A.FMT_CNS, 0x100, 3, 130, lambda t: _seq_body(A.FMT_CNS, t), None),
    "lz02": (A.FMT_LZ02, 0xFFF, 3, 272, _lz02_body, None),
    "wflz": (A.FMT_WFLZ, 0xFFFF, 5, 255, lambda t: _wflz_body(t, False), None),
    "wflz_be": (A.FMT_WFLZ_BE, 0xFFFF, 5, 255, lambda t: _wflz_body(t, True), None),
    "refpack": (A.FMT_REFPACK, 0x20000, 5, 1028, _refpack_body, None),
    "lzhudson": (A.FMT_LZHUDSON, 0x1000, 3, 273, _lzhudson_body, None),
    "smsr00": (A.FMT_SMSR00, 0x1000, 3, 18, _smsr00_item, None),
    # (PRS: a length of 2 exists in the short form only, distances up to 0x100 -- the long form's length field 0 announces a length byte, PRS.cs:83-90: 3 is the
    # shortest match at distance W)
    "prs_be": (A.FMT_PRS_BE, 0x1FFF, 3, 256, lambda t: _prs_body(t, True), None),
    "prs_le": (A.FMT_PRS_LE, 0x1FFF, 3, 256, lambda t: _prs_body(t, False), None),
    "cnx2": (A.FMT_CNX2, 0x800, 4, 35, _cnx2_body, None),
    "blz": (A.FMT_BLZ, 0x1002, 3, 18, lambda t: _flag8_body(t, _blz_token), None),       # (distance - 3 in twelve bits: 0x1002 is the farthest a token can say)
    "fastlz": (A.FMT_FASTLZ, 0x2000, 3, 264, lambda t: _fastlz_body(t, False), None),
    "fastlz_level2": (A.FMT_FASTLZ, 0x11FFF, 3, 100000, lambda t: _fastlz_body(t, True), None),
    "lzshrek": (A.FMT_LZSHREK, 0x1000, 3, 262, _lzshrek_body, None),
    "hig": (A.FMT_HIG, 0x7FFF, 4, 0xFFFF, _hig_body, None),
    "lzo": (A.FMT_LZO, 0xBFFF, 3, 100000, _lzo_body, None),
}


assert sorted({v[0] for v in EDGE_FORMATS.values()}) == list(range(A.FMT_COUNT))       # every body of the main codec


# formats whose first byte is a literal run's (WFLZ: a first block without literals and without a match is the end block, WFLZ.cs:130-159; FastLZ: the level rides on the
# first literal run, FastLZ.cs:181-198; LZO: a first byte above 17 is a literal count, LZO.cs:59-64, and the far match's opcode at distance W is 0x18 and more): no
# stream of theirs starts with a match
FIRST_IS_LITERAL = (A.FMT_WFLZ, A.FMT_WFLZ_BE, A.FMT_FASTLZ, A.FMT_LZO)


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
