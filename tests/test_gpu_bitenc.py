"""-m gpu: CRILAYLA and ALLZ written on the device (alz_bitenc_*).  Every body against the Python restatement of the managed encoders
(tests/bitenc_ref.py over tests/chain_finder_ref.py, pinned to the oracle in tests/test_bitenc_cpu.py), byte for byte, in the default and the
exact context mode; everything written read back through alz_bitlz_decode_batch.  The restatement's outputs are computed once per input."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import bitenc_ref as E
import bitlz_ref as R
import chain_finder_ref as CF
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from gpu_common import ctx
from test_gpu_bitlz import TRIPLES

pytestmark = pytest.mark.gpu
CRI, ALLZ = A.BITLZ_CRILAYLA, A.BITLZ_ALLZ
GUARD = 0xA5
MODES = ((0, "default"), (1, "exact"))
QUALITIES = (0, 2, 8, 12, 15)
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
DEFAULT = R.ALLZ_DEFAULTS


@functools.lru_cache(maxsize=None)
def ref(kind, data, quality, triple=DEFAULT):
    return E.cri_compress_headerless(data, quality) if kind == CRI else E.allz_compress_headerless(data, quality, *triple)


def unique(n, seed=0):
    """n bytes without a repeated group of three inside 64 KiB (a counter in the even bytes, a block number in the odd ones), and without one
    in common with another seed's"""
    out = bytearray(n + 2)
    for i in range(0, n + 1, 2):
        out[i], out[i + 1] = (i >> 1) & 0xFF, 0x80 | ((37 * seed + (i >> 9)) & 0x7F)
    return bytes(out[:n])


def item(kind, data, triple=DEFAULT, cap=None, name=""):
    data = bytes(data)
    return dict(kind=kind, data=data, triple=triple, cap=cap, name=name or "%s %d bytes" % (A.BITLZ_NAMES[kind], len(data)))


def pack(items, lib):
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        d = it["data"]
        cap = lib.alz_bitenc_bound(it["kind"], len(d)) if it["cap"] is None else it["cap"]
        chunks.append(d + bytes((-len(d)) % 16 + (i % 3)))                 # (ragged: sources at every residue of three)
        streams[i] = A.Stream(so, do, len(d), cap, 0xDEAD, A.allz_aux0(*it["triple"]) if it["kind"] == ALLZ else 0xBEEF, 0xF00D, it["kind"])
        so += len(chunks[-1])
        do += cap + 16 + (i % 5)                                            # (>= 16 guard bytes between the slots, bodies at every alignment)
    return streams, np.frombuffer(b"".join(chunks) + bytes(1), dtype=np.uint8).copy(), do + 64


def check(items, quality, what, modes=MODES, device=False):
    """one batch of `items`: every stream's body is the restatement's, whatever surrounds it; nothing outside the bodies is written (device form)"""
    c, lib = ctx(), _lib.load()
    streams, src, dst_bytes = pack(items, lib)
    for exact, mode in modes:
        c.set_exact_kernels(exact)
        try:
            if device:
                d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)   # (no slack behind the source: the library relocates the last streams)
                try:
                    c.h2d(d_src, src)
                    c.memset(d_dst, GUARD, dst_bytes)
                    res = c.bitenc_encode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes, quality)
                    dst = c.d2h(d_dst, dst_bytes)
                finally:
                    c.free(d_src)
                    c.free(d_dst)
            else:
                dst, res = c.bitenc_encode_batch(streams, src, dst_bytes, quality)
        finally:
            c.set_exact_kernels(0)
        bodies = []
        for i, it in enumerate(items):
            tag = "%s q%d [%s%s] stream %d (%s)" % (what, quality, mode, " device" if device else "", i, it["name"])
            want = ref(it["kind"], it["data"], quality, it["triple"])
            if it["cap"] is not None and it["cap"] < len(want):
                assert (res[i].status, res[i].dst_len) == (A.ST_OUTPUT_CAPACITY, 0), tag
                want = None                                                 # (delivers nothing; what its slot holds is unspecified, nothing behind the slot is touched)
            else:
                assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(want), len(it["data"])), "%s: status %d len %d, ref len %d" % (tag, res[i].status, res[i].dst_len, len(want))
                got = dst[streams[i].dst_off:streams[i].dst_off + len(want)].tobytes()
                if got != want:
                    k = next(k for k in range(len(want)) if got[k] != want[k])
                    raise AssertionError("%s: byte %d of %d differs (gpu %02x, ref %02x)" % (tag, k, len(want), got[k], want[k]))
            bodies.append(want)
        if device:                                                          # every byte that is no body still holds the guard
            mask = np.ones(dst_bytes, dtype=bool)
            for i, b in enumerate(bodies):
                mask[streams[i].dst_off:streams[i].dst_off + (streams[i].dst_cap if b is None else len(b))] = False
            assert (dst[mask] == GUARD).all(), "%s q%d [%s]: a byte outside the bodies was written (first at %d)" % (what, quality, mode, int(np.nonzero(mask & (dst != GUARD))[0][0]))
    return bodies


def decode_back(items, bodies):
    """the bodies through alz_bitlz_decode_batch: the inputs again"""
    n = len(items)
    streams = (A.Stream * n)()
    so, do, chunks = 0, 0, []
    for i, (it, b) in enumerate(zip(items, bodies)):
        ln = len(it["data"])
        streams[i] = A.Stream(so, do, len(b), ln, ln, A.allz_aux0(*it["triple"]), 0, it["kind"])
        chunks.append(b + bytes((-len(b)) % 16))
        so += len(chunks[-1])
        do += (ln + 15) // 16 * 16
    dst, res = ctx().bitlz_decode_batch(streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 64)
    for i, it in enumerate(items):
        assert (res[i].status, res[i].dst_len) == (A.ST_OK, len(it["data"])), (i, it["name"], res[i].status)
        assert dst[streams[i].dst_off:streams[i].dst_off + len(it["data"])].tobytes() == it["data"], (i, it["name"])


def common_inputs(test_bmp):
    rng = random.Random(1)
    out = []
    for n in LENGTHS:
        out += [("zeros %d" % n, bytes(n)), ("period-3 %d" % n, (b"abc" * (n // 3 + 1))[:n]), ("random %d" % n, bytes(rng.randrange(256) for _ in range(n)))]
    return out + [("Test.bmp[:10240]", test_bmp[:10240])]


@pytest.mark.parametrize("quality", QUALITIES)
@pytest.mark.parametrize("kind", (CRI, ALLZ))
def test_bit_identity_with_the_restatement(test_bmp, kind, quality):
    items = [item(kind, d, name=name) for name, d in common_inputs(test_bmp)]
    bodies = check(items, quality, "common inputs")
    decode_back(items, bodies)


def test_allz_quality_1_is_refused_with_the_reason():
    it = [item(ALLZ, b"abcabcabcabc"), item(CRI, b"abcabcabcabc")]
    with pytest.raises(_lib.AlzError) as e:
        check(it, 1, "quality 1", modes=MODES[:1])
    assert e.value.code == A.E_UNSUPPORTED and "quality 1" in str(e.value) and "chain table" in str(e.value)
    check(it[1:], 1, "CRILAYLA at quality 1")                               # (every quality 0..15 for CRILAYLA)


# ---------------------------------------------------------------------------------------------- CRILAYLA
SOUP_LENGTHS = (3, 4, 5, 6, 12, 13, 43, 44, 70, 298, 299, 553, 554, 600)


def cri_token_soup(extra):
    """a fixed token list -- literals, matches on both sides of every step of the length code (3-5 | 6-12 | 13-43 | 44-298 | 299-553 | ...), window
    boundaries in between -- behind `extra` literals.  The finder sees the source reversed, so this is built as the finder sees it and turned round.
    The separators differ from the bytes that would lengthen a repeat at either end."""
    u = unique(700, 3)
    parts = [unique(extra, 30), u]
    for k, ln in enumerate(SOUP_LENGTHS):
        s, s_next = 5 * k, 5 * (k + 1)
        parts += [u[s:s + ln], bytes([u[s + ln] ^ 0x55, 0x70 + k, u[s_next - 1] ^ 0x55])]
    return bytes(reversed(b"".join(parts)))


def cri_length_class(length):
    rem = length - 3
    return 0 if rem < 3 else 1 if rem < 10 else 2 if rem < 41 else 3 if rem < 296 else 4 if rem < 551 else 5


def test_crilayla_window_edge_runs_long_lengths_and_bit_phases():
    edge = []
    for n in range(8190, 8201):                                             # a repeat at distance n: taken up to 0x2000 (the field distance - 3 ends at 8189)
        u = unique(n, 1)
        edge.append(item(CRI, u + u[:9], name="repeat at distance %d" % n))
    bodies = check(edge, 8, "window edge")
    literal_only = [(9 * len(it["data"]) + 7) // 8 for it in edge]
    assert [len(b) < lo for b, lo in zip(bodies, literal_only)] == [True] * 3 + [False] * 8             # (8190 .. 8192 taken, 8193 on not)
    decode_back(edge, bodies)
    runs = [item(CRI, bytes(n), name="%d equal bytes" % n) for n in (5000,) + tuple(range(8190, 8201))]
    b0 = check(runs[:1], 0, "equal bytes")                                  # distances 1 and 2 use up the one attempt: no match at all
    assert len(b0[0]) == (5000 * 9 + 7) // 8
    decode_back(runs, check(runs, 2, "equal bytes"))
    long3 = [item(CRI, (b"xyz" * 23334)[:70000], name="period-3, 70 000 bytes")]                        # the 65 535 clamp: 257 continuation fields of eight ones
    bodies = check(long3, 0, "long match")
    assert b"\xff" * 250 in bodies[0]
    decode_back(long3, bodies)
    soup = [item(CRI, cri_token_soup(k), name="%d extra literals" % k) for k in range(8)]     # (nine bits each: every later token at every bit phase)
    seen = {m[2] for m in CF.matches(E.CRI_LZ, bytes(reversed(soup[0]["data"])), 12)}
    assert set(SOUP_LENGTHS[1:]) <= seen and {cri_length_class(ln) for ln in seen if ln} == set(range(6)), sorted(seen)
    for q in (0, 8, 12):
        decode_back(soup, check(soup, q, "bit phases"))


# ---------------------------------------------------------------------------------------------- ALLZ
STEPS = (1, 2, 3, 4, 5, 6, 7, 14, 15, 30, 31, 62, 63, 126, 127, 254, 255, 510, 511)      # run lengths on both sides of every WriteALFlag step for len_bits 0 and 1
RUNS = tuple(sorted({r + d for r in STEPS for d in (-1, 0, 1, 2)} - {0}))             # (the parse may give a neighbouring byte to a match: one more, one less)


def allz_units(runs, seed, lead=0):
    """[run][match] units: fresh bytes of each run length, then eight bytes seen before; `lead` extra bytes in the first run shift every later bit"""
    head = unique(64 + lead, seed)
    parts, k = [head], 0
    for r in (9,) + tuple(runs):                                              # (the first run joins the head's bytes: a spare one in front)
        k += 1
        parts += [unique(r, seed + 7 * k), head[8:16 + k % 5]]
    return b"".join(parts)


def test_allz_triples_run_length_steps_and_hand_over_phases(test_bmp):
    for triple in TRIPLES:
        items = [item(ALLZ, test_bmp[:10240], triple, name="Test.bmp[:10240] %r" % (triple,)), item(ALLZ, allz_units(RUNS, 2), triple, name="run steps %r" % (triple,)),
                 item(ALLZ, b"", triple, name="empty %r" % (triple,))]
        bodies = check(items, 8, "triples")
        assert bodies[2] == b"\x01"
        sp, runs = 0, set()
        for offset, _, length in CF.matches(E.ALLZ_LZ, items[1]["data"], 8):
            runs.add(offset - sp)
            sp = offset + length
        assert set(STEPS) <= runs, sorted(set(STEPS) - runs)
        decode_back(items, bodies)
    phased = [item(ALLZ, allz_units(RUNS[lead:lead + 24], 4, lead), name="lead %d" % lead) for lead in range(8)]
    phases = set()
    for it in phased:                                                       # (the restatement says at which bit of the open flag byte every run is handed over)
        seen = []
        E.allz_emit(it["data"], CF.matches(E.ALLZ_LZ, it["data"], 2), *DEFAULT, phases=seen)
        phases |= set(seen)
    assert phases == set(range(8)), phases
    decode_back(phased, check(phased, 2, "hand-over phases"))


ALLZ_TIERS = ((0x1000, 3), (0x4000, 4), (0x8000, 5), (0x20000, 6), (0x80000, 8))            # (MaxDistance, MinLength) of the five sets  ALLZ.cs:25-32


@functools.lru_cache(maxsize=None)
def allz_tier_input():
    """(data, plants): random filler with repeats of 3..8 bytes planted at distances just inside and just outside every tier of the five
    property sets; plants = (position, distance, length)"""
    rng = np.random.RandomState(7)
    data = bytearray(rng.randint(0, 256, 0x80000 + 64, dtype=np.uint8).tobytes())
    plants = []
    for tier, _ in ALLZ_TIERS:
        for d in (tier, tier + 1):
            for ln in range(3, 9):
                p = len(data)
                plants.append((p, d, ln))
                data += data[p - d:p - d + ln] + rng.randint(0, 256, 9, dtype=np.uint8).tobytes()
    return bytes(data), tuple(plants)


def allz_tier_min(distance):
    return next((mn for mx, mn in ALLZ_TIERS if distance <= mx), None)


def test_allz_length_clamp_and_distance_tiers():
    long5 = [item(ALLZ, (b"01234" * 60000)[:300000], name="period-5, 300 000 bytes")]                  # the length clamp 0x40000
    bodies = check(long5, 0, "length clamp")
    assert len(bodies[0]) < 64
    decode_back(long5, bodies)
    data, plants = allz_tier_input()
    tiers = [item(ALLZ, data, name="planted repeats")]
    decode_back(tiers, check(tiers, 0, "distance tiers"))                   # (one candidate per position and 2^15 heads for 2^19 positions: the far plants are hidden here)
    # at quality 8 the chains reach the plants.  What the reference took, so that the bytes compared below cover the rule: every match obeys its
    # tier; every tier has a plant taken at its last distance; a plant one byte further that only the nearer tier would admit is not taken;
    # nothing at all is taken beyond the window
    found = [m for m in CF.matches(E.ALLZ_LZ, data, 8) if m[2]]
    assert all(allz_tier_min(d) is not None and ln >= allz_tier_min(d) for _, d, ln in found), [m for m in found if allz_tier_min(m[1]) is None or m[2] < allz_tier_min(m[1])]

    def taken(plant):
        p, d, ln = plant
        return any(md == d and p - 1 <= mo < p + ln for mo, md, _ in found)
    for k, (tier, mn) in enumerate(ALLZ_TIERS):
        assert any(taken(pl) for pl in plants if pl[1] == tier), "no plant taken at distance 0x%x" % tier
        outer = ALLZ_TIERS[k + 1][1] if k + 1 < len(ALLZ_TIERS) else 9
        for pl in plants:
            if pl[1] == tier + 1 and pl[2] < outer:
                assert not taken(pl), "a plant of %d bytes at distance 0x%x was taken" % (pl[2], pl[1])
        if k + 1 < len(ALLZ_TIERS):
            assert any(taken(pl) for pl in plants if pl[1] == tier + 1 and pl[2] >= outer), "no plant taken at distance 0x%x" % (tier + 1)
    assert max(d for _, d, _ in found) == 0x80000
    decode_back(tiers, check(tiers, 8, "distance tiers"))


# ---------------------------------------------------------------------------------------------- batches, the device form, capacity, bounds
def mixed_items(test_bmp):
    rng = random.Random(4)
    datas = [b"", test_bmp[:3000], bytes(100), b"", bytes(rng.randrange(4) for _ in range(2500)), b"q", (b"abcd" * 700)[:2777], test_bmp[5000:5777], b"", unique(1500, 9) * 2]
    return [item((CRI, ALLZ)[(i // 2) % 2], d, TRIPLES[i % len(TRIPLES)]) for i, d in enumerate(datas)] + [item(ALLZ, b""), item(CRI, b"")]


def test_mixed_ragged_batch_and_the_device_form(test_bmp):
    items = mixed_items(test_bmp)
    host = check(items, 8, "mixed batch")
    dev = check(items, 8, "mixed batch", device=True)                       # (guard bytes everywhere outside the bodies)
    assert host == dev
    for it, b in zip(items, host):                                          # each stream alone: the same bytes
        assert check([it], 8, "alone", modes=MODES[:1]) == [b]
    decode_back(items, host)


def test_capacity_one_short_leaves_the_neighbours_and_the_canary_alone(test_bmp):
    for kind in (CRI, ALLZ):
        rng = random.Random(6)
        base = [item(kind, test_bmp[:2000]), item(kind, bytes(rng.randrange(256) for _ in range(777))), item(kind, test_bmp[2000:3000])]
        need = len(ref(kind, base[1]["data"], 8))
        for cap in (need - 1, need // 2, 0):
            items = [base[0], dict(base[1], cap=cap), base[2]]
            check(items, 8, "capacity %d of %d" % (cap, need), device=True)
        check([base[0], dict(base[1], cap=need), base[2]], 8, "capacity exact", device=True)


def test_bounds_hold_on_what_expands_most():
    lib = _lib.load()
    rng = random.Random(8)
    for n in (1, 5, 64, 1000, 5000):
        rnd = bytes(rng.randrange(256) for _ in range(n))
        items = [item(CRI, rnd), item(CRI, unique(n, 2))] + [item(ALLZ, rnd, t) for t in ((0, 0, 0), (24, 24, 24), DEFAULT)]
        for it, b in zip(items, check(items, 0, "bounds", modes=MODES[:1])):
            assert len(b) <= lib.alz_bitenc_bound(it["kind"], n), (it["name"], len(b))


def test_files_round_trip_and_match_the_restatement(test_bmp):
    cl, az = F.CRILAYLA(), F.ALLZ()
    data = test_bmp[:6000]
    f = cl.Encode(data, F.CompressionSettings(8))
    assert f == E.cri_compress(data, 8) and cl.Decompress(f) == data and R.cri_file_decode(f)[:3] == ("ok", R.OK, data)
    assert cl.Encode(bytes(0x100)) == b"CRILAYLA" + bytes(8) + bytes(0x100)                              # an empty body
    az.LzCopyBits, az.LzDistanceBits, az.LzLengthBits = 2, 8, 3
    g = az.Encode(data, F.CompressionSettings(12))
    assert g == E.allz_compress(data, 12, 2, 8, 3) and az.Decompress(g) == data
    assert R.allz_decode(g[12:], len(data), None, 2, 8, 3)[:3] == (data, R.OK, len(data))
    many = [data[:3000], bytes(300), data[100:700]]
    assert cl.EncodeMany(many) == [cl.Encode(d) for d in many] and az.EncodeMany(many + [b""]) == [az.Encode(d) for d in many + [b""]]
    short = cl.EncodeMany([bytes(0xFF), data[:1000]])
    assert isinstance(short[0], _lib.AlzError) and short[0].code == A.E_INVALID and short[1] == cl.Encode(data[:1000])
    for cls in (F.CRILAYLA, F.ALLZ):
        with pytest.raises(NotImplementedError):
            cls().Compress(data)
    # a destination one byte short: ALZ_E_NOMEM, *dst_len 0
    lib, dl = _lib.load(), C.c_size_t(7)
    dst = np.empty(len(f), dtype=np.uint8)
    st = A.Settings(8, 0, 0, 0)
    assert lib.alz_bitenc_file_compress(ctx().h, CRI, C.byref(st), 0, data, len(data), dst.ctypes.data_as(C.c_void_p), len(f) - 1, C.byref(dl)) == A.E_NOMEM and dl.value == 0
    assert lib.alz_bitenc_file_compress(ctx().h, CRI, C.byref(st), 0, data, len(data), dst.ctypes.data_as(C.c_void_p), len(f), C.byref(dl)) == 0 and dst[:dl.value].tobytes() == f


def test_refusals():
    c, lib = ctx(), _lib.load()
    src = np.frombuffer(bytes(64), dtype=np.uint8).copy()
    dst = np.empty(4096, dtype=np.uint8)
    res = (A.Result * 1)()

    def call(kind=ALLZ, aux0=A.allz_aux0(), quality=8, mwb=0, mind=0):
        s = (A.Stream * 1)(A.Stream(0, 0, 32, 2048, 0, aux0, 0, kind))
        st = A.Settings(quality, mwb, 0, mind)
        return lib.alz_bitenc_encode_batch(c.h, C.byref(st), 1, src.ctypes.data_as(C.c_void_p), 64, s, dst.ctypes.data_as(C.c_void_p), 4096, res)

    assert call() == 0 and call(CRI, 0xFFFFFFFF) == 0                       # (aux0 of a CRILAYLA stream is ignored)
    assert call(kind=2) == A.E_INVALID and call(kind=A.FMT_COUNT + 1) == A.E_INVALID
    for bad in (A.allz_aux0(25, 0, 0), A.allz_aux0(0, 25, 0), A.allz_aux0(0, 0, 25), 1 << 24):
        assert call(aux0=bad) == A.E_INVALID
    assert call(aux0=A.allz_aux0(24, 24, 24)) == 0
    assert call(quality=16) == A.E_INVALID and call(quality=-1) == A.E_INVALID
    assert call(mwb=13) == A.E_UNSUPPORTED and call(CRI, mwb=20) == A.E_UNSUPPORTED and call(mind=2) == A.E_UNSUPPORTED
    assert call(quality=1) == A.E_UNSUPPORTED and b"quality 1" in lib.alz_last_error()
    assert call(CRI, quality=1) == 0
    # the public encoder does not know the internal formats
    s = (A.Stream * 1)(A.Stream(0, 0, 32, 2048, 0, 0, 0, A.FMT_COUNT + 1))
    with pytest.raises(_lib.AlzError) as e:
        c.encode_batch(s, src, 4096)
    assert e.value.code == A.E_INVALID and "unknown format" in str(e.value)
    assert lib.alz_bitenc_file_compress(c.h, CRI, None, 0, bytes(0xFF), 0xFF, dst.ctypes.data_as(C.c_void_p), 4096, None) == A.E_INVALID
    assert lib.alz_bitenc_file_compress(c.h, 2, None, 0, bytes(0x100), 0x100, dst.ctypes.data_as(C.c_void_p), 4096, None) == A.E_INVALID
    assert lib.alz_bitenc_file_compress(c.h, ALLZ, None, A.allz_aux0(0, 0, 25), bytes(0x100), 0x100, dst.ctypes.data_as(C.c_void_p), 4096, None) == A.E_INVALID
