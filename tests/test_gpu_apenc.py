"""-m gpu: aPLib written on the device (alz_apenc_*).  Every body against the Python restatement of the managed encoder (tests/apenc_ref.py over
tests/chain_finder_ref.py, pinned in tests/test_apenc_cpu.py), byte for byte, in the default (one wavefront per stream) and the exact (one lane)
context mode; what is written is read back through alz_aplib_decode_batch.  The restatement's outputs are computed once per input; the inputs
above 256 KiB compare hashes with tests/golden/apenc_far.json."""
import ctypes as C
import functools
import hashlib
import json
import os
import random
import sys

import numpy as np
import pytest

import apenc_ref as E
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_apenc_kats as KATS  # noqa: E402

GUARD = 0xA5
MODES = ((0, "default"), (1, "exact"))
LENGTHS = (1, 2, 3, 4, 5, 8, 63, 64, 65, 127, 128, 129)
MATCH_KINDS = ("rep", "short", "match", "match_biased")


@functools.lru_cache(maxsize=None)
def ref(data, quality, strategy=0):
    return E.compress_headerless(data, quality, strategy)


@functools.lru_cache(maxsize=None)
def traced(data, quality):
    t = []
    E.compress_headerless(data, quality, 0, None, t)
    return tuple(t)


def item(data, cap=None, name=""):
    data = bytes(data)
    return dict(data=data, cap=cap, name=name or "%d bytes" % len(data))


def pack(items, lib, tight=False):
    """sources at every residue of three, >= 16 guard bytes between the slots, bodies at every alignment; tight: the last source ends at the buffer's end"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        d = it["data"]
        cap = lib.alz_apenc_bound(len(d)) if it["cap"] is None else it["cap"]
        chunks.append(d if (tight and i == n - 1) else d + bytes((-len(d)) % 16 + (i % 3)))
        streams[i] = A.Stream(so, do, len(d), cap, 0xDEAD, 0xBEEF, 0xF00D, 0x77)   # (decom_len, aux0, aux1 and format are ignored)
        so += len(chunks[-1])
        do += cap + 16 + (i % 5)
    return streams, np.frombuffer(b"".join(chunks) + (b"" if tight else bytes(1)), dtype=np.uint8).copy(), do + 64


def run(items, quality, modes=MODES, device=False, strategy=0, tight=False):
    """one batch of `items` per mode -> [(results, dst, streams)]"""
    c, lib = ctx(), _lib.load()
    streams, src, dst_bytes = pack(items, lib, tight)
    out = []
    for exact, mode in modes:
        c.set_exact_kernels(exact)
        try:
            if device:
                d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)   # (no slack behind the source: the library relocates the last streams)
                try:
                    c.h2d(d_src, src)
                    c.memset(d_dst, GUARD, dst_bytes)
                    res = c.apenc_encode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes, quality, strategy)
                    dst = c.d2h(d_dst, dst_bytes)
                finally:
                    c.free(d_src)
                    c.free(d_dst)
            else:
                dst, res = c.apenc_encode_batch(streams, src, dst_bytes, quality, strategy)
        finally:
            c.set_exact_kernels(0)
        out.append((res, dst, streams, mode))
    return out, dst_bytes


def check(items, quality, what, modes=MODES, device=False, strategy=0, tight=False):
    """every stream's body is the restatement's, whatever surrounds it; nothing outside the bodies is written (device form)"""
    runs, dst_bytes = run(items, quality, modes, device, strategy, tight)
    bodies = None
    for res, dst, streams, mode in runs:
        bodies = []
        for i, it in enumerate(items):
            tag = "%s q%d s%d [%s%s] stream %d (%s)" % (what, quality, strategy, mode, " device" if device else "", i, it["name"])
            want = ref(it["data"], quality, strategy)
            if it["cap"] is not None and it["cap"] < len(want):
                assert (res[i].status, res[i].dst_len) == (A.ST_OUTPUT_CAPACITY, 0), tag
                want = None
            else:
                assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(want), len(it["data"])), "%s: status %d len %d, ref len %d" % (tag, res[i].status, res[i].dst_len, len(want))
                got = dst[streams[i].dst_off:streams[i].dst_off + len(want)].tobytes()
                if got != want:
                    k = next(k for k in range(len(want)) if got[k] != want[k])
                    raise AssertionError("%s: byte %d of %d differs (gpu %02x, ref %02x)" % (tag, k, len(want), got[k], want[k]))
            bodies.append(want)
        if device:                                                          # every byte that is no body still holds the guard: a refused stream's slot too
            mask = np.ones(dst_bytes, dtype=bool)
            for i, b in enumerate(bodies):
                if b is not None:
                    mask[streams[i].dst_off:streams[i].dst_off + len(b)] = False
            assert (dst[mask] == GUARD).all(), "%s q%d [%s]: a byte outside the bodies was written (first at %d)" % (what, quality, mode, int(np.nonzero(mask & (dst != GUARD))[0][0]))
    return bodies


def decode_back(items, bodies):
    """the bodies through alz_aplib_decode_batch: the inputs again, src_used == the body's length"""
    n = len(items)
    streams = (A.Stream * n)()
    so, do, chunks = 0, 0, []
    for i, (it, b) in enumerate(zip(items, bodies)):
        ln = len(it["data"])
        streams[i] = A.Stream(so, do, len(b), ln, 0, 0, 0, 0)
        chunks.append(b + bytes((-len(b)) % 16))
        so += len(chunks[-1])
        do += (ln + 15) // 16 * 16
    dst, res = ctx().aplib_decode_batch(streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 64)
    for i, it in enumerate(items):
        assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(it["data"]), len(bodies[i])), (i, it["name"], res[i].status, res[i].dst_len, res[i].src_used)
        assert dst[streams[i].dst_off:streams[i].dst_off + len(it["data"])].tobytes() == it["data"], (i, it["name"])


def noise(n, seed, lo=1, hi=200):
    """n bytes lo..hi-1 from a seeded generator: no zero, few equal bytes within fifteen, hardly a repeat"""
    rng = random.Random(seed)
    return bytes(rng.randrange(lo, hi) for _ in range(n))


def ramp(n):
    return bytes(1 + (i % 255) for i in range(n))


# ---------------------------------------------------------------------------------------------- the smallest shapes
def small_inputs():
    rng = random.Random(1)
    out = []
    for n in LENGTHS:
        out += [("zeros %d" % n, bytes(n)), ("ramp %d" % n, ramp(n)), ("two symbols %d" % n, bytes(rng.choice(b"\x11\x7e") for _ in range(n)))]
    return out


def lookback_inputs():
    """a byte equal to the one 1, 15 and 16 positions back (16 is outside the look-back: a literal), a zero byte, and each of them at positions 1..3"""
    out = []
    base = ramp(40)
    for back in (1, 15, 16):
        d = bytearray(base)
        d[30] = d[30 - back]
        out.append(("equal %d back" % back, bytes(d)))
    d = bytearray(base)
    d[30] = 0
    out.append(("a zero byte", bytes(d)))
    for pos in (1, 2, 3):
        for back in range(1, pos + 1):
            d = bytearray(base[:8])
            d[pos] = d[pos - back]
            out.append(("position %d equals %d back" % (pos, back), bytes(d)))
        d = bytearray(base[:8])
        d[pos] = 0
        out.append(("zero at position %d" % pos, bytes(d)))
        out.append(("%d bytes ending in a zero" % (pos + 1), bytes(d[:pos + 1])))
    return out


@pytest.mark.parametrize("quality", (0, 8, 12))
def test_smallest_shapes_and_the_look_back(quality):
    items = [item(d, name=name) for name, d in small_inputs() + lookback_inputs()]
    bodies = check(items, quality, "small")
    decode_back(items, bodies)
    if quality == 8:
        kinds = {name: [t[0] for t in traced(d, 8)] for name, d in lookback_inputs()}
        assert kinds["equal 1 back"].count("one") == 1 and kinds["equal 15 back"].count("one") == 1 and kinds["equal 16 back"].count("one") == 0 and kinds["a zero byte"].count("one") == 1
        assert all(kinds["position %d equals %d back" % (p, b)].count("one") == 1 for p in (1, 2, 3) for b in range(1, p + 1))


def test_long_runs():
    """70 000 equal bytes: one match whose length gamma has 2 * 16 bits (the length goes through the entry behind the match's); 1 MiB of zeros"""
    items = [item(b"\x5a" * 70000, name="70 000 equal bytes"), item(bytes(1 << 20), name="1 MiB of zeros")]
    for q in (0, 8):
        bodies = check(items, q, "runs")
        assert len(bodies[0]) < 16 and len(bodies[1]) < 16
    decode_back(items, bodies)
    assert [t[4] for t in traced(items[0]["data"], 8) if t[0] in MATCH_KINDS] == [69999]


# ---------------------------------------------------------------------------------------------- the emitter's window seams
def seam_input(variant):
    """Noise with planted repeats at the places where a 64-position window of the emitter ends.  `variant` 0..7 changes the BITS in front of them and not the
    positions: zero bytes (7 bits where a literal has 1) and a five-byte repeat (6 bits where five literals have 5) in the first 48 bytes."""
    d = bytearray(noise(1400, 42))       # (a seed whose first 48 bytes are literals only, so that the eight variants are the eight phases: asserted below)
    for k in range(variant // 2):
        d[6 + 7 * k] = 0
    if variant & 1:
        d[36:41] = d[28:33]
    def plant(at, dist, length):
        d[at:at + length] = d[at - dist:at - dist + length]
    plant(127, 40, 6)                    # a match starting at lane 63
    plant(186, 50, 6)                    # a match ending exactly at 192 ...
    plant(192, 70, 7)                    # ... followed by a match: lwm across the seam
    plant(250, 33, 6)                    # distance 33, then two whole windows of literals ...
    plant(460, 33, 9)                    # ... and the same distance again: a repeat whose lastOffset comes from windows back
    plant(600, 300, 250)                 # a match that covers several windows
    plant(1023, 90, 1)                   # (a one-byte match in lane 63 ...
    d[1024] = 0                          #  ... and one in lane 0)
    plant(1150, 23, 5)                   # a match in front of a seam, a literal behind it
    return bytes(d)


def test_window_seams_at_every_flag_phase():
    items = [item(seam_input(v), name="variant %d" % v) for v in range(8)]
    phases = {k: set() for k in ("lane 63", "lwm seam", "repeat", "long")}
    for it in items:
        tr = traced(it["data"], 8)
        ms = [t for t in tr if t[0] in MATCH_KINDS]
        for j, (kind, pos, bits, dist, length) in enumerate(ms):
            if pos % 64 == 63:
                phases["lane 63"].add(bits % 8)
            if kind == "match" and pos % 64 == 0 and j and ms[j - 1][1] + ms[j - 1][4] == pos:
                phases["lwm seam"].add(bits % 8)
            if kind == "rep" and j and pos // 64 - (ms[j - 1][1] + ms[j - 1][4]) // 64 >= 2:
                phases["repeat"].add(bits % 8)
            if length >= 192:
                phases["long"].add(bits % 8)
    assert all(p == set(range(8)) for p in phases.values()), phases
    for q in (8, 10):
        decode_back(items, check(items, q, "seams"))


# ---------------------------------------------------------------------------------------------- LengthDelta, the short form, the high part's gamma, the sets
def planted_input(plants, size, seed, gap=11):
    """noise below 200 with, per (distance, length, adjacent), `length` bytes of 200 and above written `distance` back and copied to the end -- behind `gap` bytes
    of noise, or (adjacent) right behind the plant before it"""
    rng = random.Random(seed)
    d = bytearray(noise(size, seed))
    for dist, length, adjacent in plants:
        if not adjacent:
            d += noise(gap, rng.randrange(1 << 30))
        p = len(d)
        seg = bytes(rng.randrange(200, 256) for _ in range(length))
        d[p - dist:p - dist + length] = seg
        d += seg
    return bytes(d) + noise(gap, seed + 1)


# (in rounds, so that no plant has the distance of the one before it: that would be a repeat)
EDGE_PLANTS = [(127, 2), (128, 2), (0x4FF, 3), (0x500, 3), (0x7CFF, 5), (0x7D00, 5), (127, 3), (128, 3), (0x4FF, 4), (0x500, 4), (0x7CFF, 6), (0x7D00, 6),
               (127, 4), (128, 4), (0x4FF, 9), (0x500, 9), (0x7CFF, 12), (0x7D00, 12), (127, 9), (128, 9)]


@functools.lru_cache(maxsize=None)
def edge_input():
    return planted_input([(d, ln, False) for d, ln in EDGE_PLANTS], 0x7D00 + 64, 3, gap=150)   # (a gap wider than 128: a near plant's source lies in its own gap, not in the plant before it)


def test_length_delta_and_short_form_edges():
    """D in {127, 128, 0x4FF, 0x500, 0x7CFF, 0x7D00} with L at the set's minimum and above (quality 10: two and three bytes come from the min-length table)"""
    data = edge_input()
    taken = {(t[3], t[4]): t[0] for t in traced(data, 10) if t[0] in MATCH_KINDS}
    for d, ln in EDGE_PLANTS:
        assert (d, ln) in taken, "the plant (0x%x, %d) was not taken" % (d, ln)
        assert (taken[(d, ln)] == "short") == (ln <= 3 and d <= 127), (d, ln, taken[(d, ln)])
    items = [item(data, name="edges")]
    decode_back(items, check(items, 10, "LengthDelta edges"))
    decode_back(items, check(items, 8, "LengthDelta edges"))


HIGH_PARTS = (1, 2, 5, 6, 13, 14, 29, 30, 61, 62, 125, 126, 253, 254, 509, 510, 1021, 1022)          # (D >> 8) + 2 and + 3 on both sides of 4, 8, ..., 1024
SET_EDGES = ((0x1000, 3), (0x4000, 4), (0x10000, 5), (0x40000, 6))                                      # sets 0, 2, 3, 4: (MaxDistance, MinLength); set 1 (0x80, 2..3) is among the edges above


@functools.lru_cache(maxsize=None)
def wide_input():
    plants = []
    for h in HIGH_PARTS:
        plants += [((h << 8) | 0x35, 8, False), ((h << 8) | 0xC1, 8, True)]                             # a pair: the first after a literal (the bias), the second right behind it (lwm)
    for mx, mn in SET_EDGES:
        plants += [(mx, mn, False), (mx, mn - 1, False), (mx + 1, mn, False), (mx + 1, mn + 1, False)]
    return planted_input(plants, 0x40000 + 64, 5, gap=40), tuple(plants)                                 # (seed and gap such that no plant's source falls on another plant: asserted by the test)


def test_high_part_gammas_and_set_edges_up_to_0x40000():
    data, plants = wide_input()
    tr = traced(data, 10)
    taken = {(t[3], t[4]): t[0] for t in tr if t[0] in MATCH_KINDS}
    for h in HIGH_PARTS:
        assert taken.get(((h << 8) | 0x35, 8)) == "match_biased" and taken.get(((h << 8) | 0xC1, 8)) == "match", (h, taken.get(((h << 8) | 0x35, 8)), taken.get(((h << 8) | 0xC1, 8)))
    for mx, mn in SET_EDGES:                                                 # the last admitted distance with the minimum length: taken; one byte less, or one further: not; one further with the next set's minimum: taken
        assert (mx, mn) in taken and (mx, mn - 1) not in taken and (mx + 1, mn) not in taken and (mx + 1, mn + 1) in taken, (hex(mx), mn)
    items = [item(data, name="high parts and set edges")]
    decode_back(items, check(items, 10, "wide"))


def test_far_sets_from_the_golden_file():
    """the 0x100000 and 0x200000 edges: a match at distance exactly 0x200000, none at 0x200001 -- the body's SHA-256 is the restatement's (tests/golden/apenc_far.json)"""
    kat = json.load(open(os.path.join(HERE, "golden", "apenc_far.json")))["far"]
    data = KATS.build(kat["params"])
    assert len(data) == kat["input_len"] and hashlib.sha256(data).hexdigest() == kat["input_sha256"]
    assert [0x200000, 8] in kat["far_matches"] and not [m for m in kat["far_matches"] if m[0] > 0x200000]
    items = [item(data, name="far")]
    runs, _ = run(items, kat["params"]["quality"])
    for res, dst, streams, mode in runs:
        assert (res[0].status, res[0].dst_len, res[0].src_used) == (A.ST_OK, kat["body_len"], len(data)), (mode, res[0].status, res[0].dst_len)
        body = dst[streams[0].dst_off:streams[0].dst_off + res[0].dst_len].tobytes()
        assert hashlib.sha256(body).hexdigest() == kat["body_sha256"], mode
    decode_back(items, [body])


# ---------------------------------------------------------------------------------------------- qualities, strategies, the chain table's size
@pytest.mark.parametrize("quality", (0, 1, 4, 7, 8, 10, 12, 15))
def test_qualities(test_bmp, quality):
    rng = random.Random(3)
    items = [item(test_bmp[:10240], name="Test.bmp[:10240]"), item(bytes(rng.randrange(4) for _ in range(5000)), name="four symbols")]
    decode_back(items, check(items, quality, "qualities"))


def test_both_strategies(test_bmp):
    items = [item(test_bmp[:10240], name="Test.bmp[:10240]"), item((b"abcde" * 900)[:4321], name="period 5"), item(bytes(3000), name="zeros")]
    b0, b1 = check(items, 8, "strategy", strategy=0), check(items, 8, "strategy", strategy=1)
    assert b0 != b1                      # (noSelfOverlap cuts a run's match at its distance)
    decode_back(items, b1)


def test_quality_1_and_the_chain_table():
    """2^18 slots at quality 1: a stream of exactly that many bytes is written, one byte more makes the whole call ALZ_E_UNSUPPORTED with nothing written"""
    big = noise(1 << 18, 9)
    big = big[:1000] * 40 + big[40000:]                                      # (some matches too)
    items = [item(big, name="1 << 18 bytes"), item(b"abcabcabc", name="nine bytes")]
    decode_back(items, check(items, 1, "quality 1", modes=MODES[:1]))
    c, lib = ctx(), _lib.load()
    over = [item(big + b"x", name="(1 << 18) + 1 bytes"), items[1]]
    streams, src, dst_bytes = pack(over, lib)
    dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
    with pytest.raises(_lib.AlzError) as e:
        c.apenc_encode_batch(streams, src, dst_bytes, 1, 0, dst=dst)
    assert e.value.code == A.E_UNSUPPORTED and "quality 1" in str(e.value) and "chain table" in str(e.value)
    assert (dst == GUARD).all()
    check(over, 8, "the same streams at quality 8", modes=MODES[:1])
    check(over, 0, "the same streams at quality 0", modes=MODES[:1])


# ---------------------------------------------------------------------------------------------- batches, the device form, capacity
def mixed_items(test_bmp):
    rng = random.Random(4)
    items = []
    for i in range(200):
        n = 1 + (i * 4001 // 200 + 37 * i) % 4000
        kind = i % 4
        d = test_bmp[97 * i:97 * i + n] if kind == 0 else bytes(rng.randrange(3) for _ in range(n)) if kind == 1 else noise(n, i) if kind == 2 else (bytes([i & 0xFF, 7, 0]) * (n // 3 + 1))[:n]
        items.append(item(d))
    items += [item(b"z"), item(test_bmp[:4000])]
    return items


def test_mixed_ragged_batch_host_and_device(test_bmp):
    items = mixed_items(test_bmp)
    assert 1 in {len(it["data"]) for it in items} and max(len(it["data"]) for it in items) == 4000
    host = check(items, 8, "mixed batch")                                    # (default and exact: the same bytes as the restatement's, so as each other's)
    dev = check(items, 8, "mixed batch", device=True, tight=True)            # (the last stream ends at the buffer's end; guard bytes everywhere outside the bodies)
    assert host == dev
    decode_back(items, host)


def test_capacity_exact_and_one_short(test_bmp):
    base = [item(test_bmp[:2000]), item(noise(777, 6)), item(test_bmp[2000:3000]), item(b"q")]
    for k in (1, 3):
        need = len(ref(base[k]["data"], 8))
        exact = [dict(it, cap=need) if j == k else it for j, it in enumerate(base)]
        check(exact, 8, "capacity exact", device=True)
        for cap in (need - 1, need // 2, 0):
            short = [dict(it, cap=cap) if j == k else it for j, it in enumerate(base)]
            check(short, 8, "capacity %d of %d" % (cap, need), device=True)  # (OUTPUT_CAPACITY, dst_len 0, the guard bytes of the slot and on both sides of it untouched)


def test_bound_is_tight_on_literals_only():
    lib = _lib.load()
    items = [item(ramp(n)) for n in (1, 8, 64, 200)] + [item(noise(3000, 2, 0, 256))]
    for it, b in zip(items, check(items, 0, "bound", modes=MODES[:1])):
        assert len(b) <= lib.alz_apenc_bound(len(it["data"]))
    assert [len(ref(it["data"], 0)) for it in items[:3]] == [3, 11, 74]


def test_refusals():
    c, lib = ctx(), _lib.load()
    src = np.frombuffer(noise(64, 1), dtype=np.uint8).copy()
    dst = np.full(4096, GUARD, dtype=np.uint8)
    res = (A.Result * 2)()

    def call(quality=8, mwb=0, mind=0, strategy=0, len1=16, settings=True):
        s = (A.Stream * 2)(A.Stream(0, 0, 32, 1024, 0, 0, 0, 0), A.Stream(32, 2048, len1, 1024, 0, 0, 0, 0))
        st = A.Settings(quality, mwb, strategy, mind)
        return lib.alz_apenc_encode_batch(c.h, C.byref(st) if settings else None, 2, src.ctypes.data_as(C.c_void_p), 64, s, dst.ctypes.data_as(C.c_void_p), 4096, res)

    assert call() == 0 and call(strategy=1) == 0
    first = dst[:res[0].dst_len].tobytes()
    assert call(settings=False) == 0 and dst[:res[0].dst_len].tobytes() == first == ref(src[:32].tobytes(), 8)        # NULL settings: quality 8
    dst[:] = GUARD
    assert call(len1=0) == A.E_INVALID and b"empty" in lib.alz_last_error()
    assert call(quality=16) == A.E_INVALID and call(quality=-1) == A.E_INVALID
    assert call(mwb=12) == A.E_UNSUPPORTED and call(mind=2) == A.E_UNSUPPORTED
    assert (dst == GUARD).all()
    assert lib.alz_apenc_encode_batch(c.h, None, 0, None, 0, None, None, 0, None) == 0                               # n == 0
    # the public encoder does not know the internal format
    s = (A.Stream * 1)(A.Stream(0, 0, 32, 2048, 0, 0, 0, A.FMT_COUNT + 3))
    with pytest.raises(_lib.AlzError) as e:
        c.encode_batch(s, src, 4096)
    assert e.value.code == A.E_INVALID and "unknown format" in str(e.value)


def test_kernel_time_is_reported(test_bmp):
    check([item(test_bmp[:5000])], 8, "kernel time", modes=MODES[:1])
    assert ctx().last_kernel_ms() > 0


# ---------------------------------------------------------------------------------------------- the file forms, the class
def test_files_round_trip_and_match_the_restatement(test_bmp):
    ap, lib = F.APLib(), _lib.load()
    data = test_bmp[:6000]
    f = ap.Encode(data, F.CompressionSettings(8))
    assert f == E.compress(data, 8)
    assert f[:4] == b"AP32" and [int.from_bytes(f[4 + 4 * k:8 + 4 * k], "little") for k in range(5)] == [24, len(f) - 24, 0, len(data), 0]
    assert ap.IsMatch(f) and ap.GetDecompressedSize(f) == len(data) and ap.Decompress(f) == data
    tiny = ap.Encode(b"x")                                                   # 24 + 3 bytes: longer than 16, so a match
    assert tiny == E.compress(b"x", 8) and len(tiny) == 27 and ap.IsMatch(tiny) and ap.Decompress(tiny) == b"x"
    g = ap.Encode(data, F.CompressionSettings(12))
    assert g == E.compress(data, 12) and ap.Decompress(g) == data
    many = [data[:3000], bytes(300), b"", data[100:700], b"y"]
    got = ap.EncodeMany(many)
    assert isinstance(got[2], _lib.AlzError) and got[2].code == A.E_INVALID                                          # an empty file fails alone
    assert [g for k, g in enumerate(got) if k != 2] == [ap.Encode(d) for k, d in enumerate(many) if k != 2]
    with pytest.raises(_lib.AlzError) as e:
        ap.Encode(b"")
    assert e.value.code == A.E_INVALID
    with pytest.raises(NotImplementedError) as ne:
        ap.Compress(data)
    assert "LzChainMatchFinder" in str(ne.value) and "oracle" in str(ne.value) and "Encode" in str(ne.value)
    assert F.APLib not in F.ALL_FORMATS
    # a destination one byte short: ALZ_E_NOMEM, *dst_len 0
    dl = C.c_size_t(7)
    dst = np.empty(len(f), dtype=np.uint8)
    st = A.Settings(8, 0, 0, 0)
    assert lib.alz_apenc_file_compress(ctx().h, C.byref(st), data, len(data), dst.ctypes.data_as(C.c_void_p), len(f) - 1, C.byref(dl)) == A.E_NOMEM and dl.value == 0
    assert lib.alz_apenc_file_compress(ctx().h, C.byref(st), data, len(data), dst.ctypes.data_as(C.c_void_p), len(f), C.byref(dl)) == 0 and dst[:dl.value].tobytes() == f
    # in the batch a slot one byte short is that file's rc, and its neighbours are written
    files = (A.Stream * 3)(A.Stream(0, 0, 3000, 4096, 0, 0, 0, 0), A.Stream(0, 4096, 6000, len(f) - 1, 0, 0, 0, 0), A.Stream(100, 12288, 600, 1024, 0, 0, 0, 0))
    out, fr = ctx().apenc_file_compress_batch(files, np.frombuffer(data, dtype=np.uint8), 16384)
    assert [r.rc for r in fr] == [0, A.E_NOMEM, 0] and fr[1].dst_len == 0
    assert out[:fr[0].dst_len].tobytes() == got[0] and out[12288:12288 + fr[2].dst_len].tobytes() == got[3]
