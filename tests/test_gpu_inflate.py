"""-m gpu: DEFLATE (alz_inflate_*, alz_zlib_*, alz_gzip_*) on the device.  Every batch goes through the host and the device entry points in
all three context modes and through both measure entry points; every result field and every output byte is held against the pure-Python
reference decoder (tests/inflate_ref.py), the hand-assembled known answers (tests/golden/inflate_kat.json) and, for valid streams, the
standard library's zlib.  Every destination lies between guard bytes.  Every comparison is exact."""
import ctypes as C
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

import inflate_ref as R
import test_inflate_cpu as IC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
MODES = ((1, 0, "exact"), (0, 1, "variant 1"), (0, 0, "default"))           # (alz_ctx_set_exact_kernels, alz_ctx_set_kernel_variant): one kernel serves all
GUARD = 0xA5


# ---------------------------------------------------------------------------------------------- helpers
def item(src, cap=None, name="", want=None):
    """one stream and the reference decoder's answer (status, output, src_used), computed once; cap None: what it decodes to, + 8"""
    src = bytes(src)
    if want is None:
        want = R.decode(src, R.NO_BOUND if cap is None else cap)
    if cap is None:
        cap = len(want[1]) + 8
    return dict(src=src, cap=cap, name=name, want=want)


def valid(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, name=""):
    """a stream the standard library wrote: the answer is the data itself"""
    s = IC.raw_deflate(data, level, strategy)
    return item(s, None, name or "zlib %d bytes level %d" % (len(data), level), want=(R.OK, bytes(data), len(s)))


def pack(items):
    """(streams, src array, dst_bytes): stream i sits at residue i mod 16 on both sides and its destination starts 1..16 bytes behind the end of
    its neighbour's capacity -- the gap is guard bytes"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        b, mis = it["src"], i % 16
        chunks.append(bytes([0xEE]) * mis + b + bytes([0xEE]) * ((-(len(b) + mis)) % 16))
        do += 1
        do += (i % 16 - do) % 16
        streams[i] = A.Stream(so + mis, do, len(b), it["cap"], 0xDEAD, 0xBEEF, 0xF00D, 77)          # (decom_len, aux0, aux1, format are ignored)
        so += len(chunks[-1])
        do += it["cap"]
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 16 + 64


def compare(tag, r, it, got_bytes):
    status, out, src_used = it["want"]
    assert (r.status, r.dst_len) == (status, len(out)), "%s: gpu status=%d len=%d used=%d | ref status=%d len=%d used=%s" % (
        tag, r.status, r.dst_len, r.src_used, status, len(out), src_used)
    if src_used is not None:
        assert r.src_used == src_used, "%s: src_used gpu %d ref %d" % (tag, r.src_used, src_used)
    if got_bytes is not None and got_bytes != out:
        d = next(k for k in range(len(out)) if got_bytes[k] != out[k])
        raise AssertionError("%s: byte %d of %d differs (gpu %d, ref %d)" % (tag, d, len(out), got_bytes[d], out[d]))


def select(exact, variant):
    ctx().set_exact_kernels(exact)
    ctx().set_kernel_variant(variant)


def check(items, what):
    """In every context mode: the host form, the device form on a destination full of guard bytes (nothing outside [dst_off, dst_off + dst_len)
    is written), and both measure forms -- measure == decode in status, dst_len, and src_used where it is defined."""
    streams, src, dst_bytes = pack(items)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        for exact, variant, mode in MODES:
            select(exact, variant)
            try:
                h_dst, h_res = c.inflate_decode_batch(streams, src, dst_bytes)
                c.memset(d_dst, GUARD, dst_bytes)
                d_res = c.inflate_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
                assert c.last_kernel_ms() > 0
                dst = c.d2h(d_dst, dst_bytes)
                m_res = c.inflate_measure_batch(streams, src)
                md_res = c.inflate_measure_batch_device(streams, d_src, src.nbytes)
            finally:
                select(0, 0)
            mask = np.ones(dst.size, dtype=bool)
            for i, it in enumerate(items):
                a, n = streams[i].dst_off, len(it["want"][1])
                assert a % 16 == i % 16 and streams[i].src_off % 16 == i % 16
                tag = "%s [%s] stream %d (%s)" % (what, mode, i, it["name"])
                compare(tag + " host", h_res[i], it, h_dst[a:a + n].tobytes())
                compare(tag + " device", d_res[i], it, dst[a:a + n].tobytes())
                compare(tag + " measure", m_res[i], it, None)
                compare(tag + " measure device", md_res[i], it, None)
                if it["want"][2] is not None:
                    assert h_res[i].src_used == d_res[i].src_used == m_res[i].src_used == md_res[i].src_used, tag
                mask[a:a + n] = False
            assert (dst[mask] == GUARD).all(), "%s [%s]: %d guard bytes overwritten, first at %d" % (
                what, mode, int((dst[mask] != GUARD).sum()), int(np.nonzero(mask & (dst != GUARD))[0][0]))
        assert np.array_equal(c.d2h(d_src, src.nbytes), src)                                       # (nothing writes the source)
    finally:
        c.free(d_src)
        c.free(d_dst)


def stream(*blocks, fill=0):
    """blocks: callables that take the BitWriter"""
    w = R.BitWriter()
    for b in blocks:
        b(w)
    return w.bytes(fill)


def zlib_agrees(it):
    """the standard library on a stream the assembler wrote: error exactly for BAD_TOKEN, the same bytes otherwise"""
    o = zlib.decompressobj(-15)
    try:
        z, err = o.decompress(it["src"]), False
    except zlib.error:
        z, err = None, True
    st, out, _ = it["want"]
    return err == (st == R.BAD) and (err or (z == out and o.eof == (st == R.OK)))


PRELUDE = bytes((131 * i * i + 7 * i + 3) % 251 + 1 for i in range(251))                         # 251 non-zero bytes, no short period


def prelude(total):
    """tokens that produce `total` >= 251 bytes: 251 literals, then matches at distance 251"""
    toks, n = [("lit", b) for b in PRELUDE], 251
    while n < total:
        L = min(258, total - n)
        if L < 3:
            toks += [("lit", 0x20 + k) for k in range(L)]
        else:
            toks.append(("match", L, 251))
        n += L
    return toks


# ---------------------------------------------------------------------------------------------- known answers
def test_all_kats():
    items = []
    for c in IC.kats():
        items.append(item(bytes.fromhex(c["src"]), c["cap"], c["name"], want=(c["status"], bytes.fromhex(c["out"]), c["src_used"])))
    check(items, "kat")


# ---------------------------------------------------------------------------------------------- match geometry
def test_match_geometry():
    """one stream of about 40 KiB in a fixed block: every length symbol and every distance symbol at its smallest and largest extra bits,
    overlapping copies at several phases, distance == produced, distance 32768; and the streams one byte too far back"""
    toks = [("lit", 0x61), ("lit", 0x62), ("match", 3, 2)]                                        # distance == bytes produced
    toks += prelude(33000)[3:]                                                                    # (the first three bytes are there)
    for sym in range(257, 286):
        eb = R.LEN_EXTRA[sym - 257]
        for ev in (0, (1 << eb) - 1):
            toks += [("len", sym, ev), ("dist", 9, 3), ("lit", sym & 0xFF)]
    for d in range(30):
        eb = R.DIST_EXTRA[d]
        for ev in (0, (1 << eb) - 1):
            toks += [("len", 260, 0), ("dist", d, ev), ("lit", 0x80 + d)]
    toks += [("match", 258, 1), ("lit", 0x41)]
    for d in (2, 3, 5, 7, 63, 64, 65):
        for L in (d + 1, 2 * d + 1, 258):
            toks += [("match", min(max(L, 3), 258), d), ("lit", 0x42)]
    toks += [("match", 100, 32768), ("lit", 0x43), ("match", 258, 32768)]
    big = item(stream(lambda w: R.fixed_block(w, toks, True)), name="geometry")
    assert big["want"][0] == R.OK and 39000 <= len(big["want"][1]) <= 48000 and zlib_agrees(big)
    items = [big]
    # distance == produced + 1, at the start and at the window's edge
    items.append(item(stream(lambda w: R.fixed_block(w, [("lit", 1), ("lit", 2), ("match", 3, 3)], True)), name="distance 3 with 2 bytes"))
    items.append(item(stream(lambda w: R.fixed_block(w, [("match", 3, 1)], True)), name="a match first"))
    items.append(item(stream(lambda w: R.fixed_block(w, prelude(32767) + [("match", 10, 32768)], True)), name="distance 32768 with 32767 bytes"))
    items.append(item(stream(lambda w: R.fixed_block(w, prelude(32768) + [("match", 10, 32768)], True)), name="distance 32768 with 32768 bytes"))
    assert [it["want"][0] for it in items[1:]] == [R.BAD, R.BAD, R.BAD, R.OK] and len(items[3]["want"][1]) == 32767
    assert all(zlib_agrees(it) for it in items)
    check(items, "geometry")


# ---------------------------------------------------------------------------------------------- dynamic tables
def _dyn(tokens, lit, dist, final=True, end=True, **header):
    return lambda w: R.dynamic_block(w, tokens, final, lit, dist, end=end, **header)


def test_dynamic_tables():
    items = []
    # literal/length code lengths 1..15 in one set (1, 2, ..., 14, 15, 15): codes longer than the 9-bit table index
    syms = [0x65, 0x20, 0x74, 0x61, 257, 0x6F, 0x6E, 256, 0x69, 0x73, 0x72, 0x68, 0x0A, 270, 0xFF, 285]
    lit = [0] * 286
    for k, s in enumerate(syms):
        lit[s] = min(k + 1, 15)
    assert R.kraft(lit) == 32768
    toks = [("lit", s) for s in syms if s < 256] * 3 + [("match", 3, 1), ("len", 270, 3), ("dist", 0, 0), ("match", 258, 2)] + [("lit", s) for s in syms if s < 256]
    items.append(item(stream(_dyn(toks, lit, [2, 2, 2, 2])), name="lengths 1..15"))
    # a single distance code, used and mis-used (the other 1-bit code)
    lit1, _ = R.lens_for([("lit", 0x41), ("lit", 0x42), ("match", 3, 1)])
    items.append(item(stream(_dyn([("lit", 0x41), ("match", 3, 1), ("lit", 0x42)], lit1, [1])), name="single distance code, used"))
    items.append(item(stream(_dyn([("lit", 0x41), ("len", 257, 0), ("bits", 1, 1), ("lit", 0x42)], lit1, [1])), name="single distance code, the unused code"))
    items.append(item(stream(_dyn([("lit", 0x41), ("len", 257, 0), ("dist", 3, 0)], lit1, [0, 0, 0, 1])), name="single distance code on symbol 3, distance 4 > produced"))
    # no distance code: literals only; and a length symbol met
    items.append(item(stream(_dyn([("lit", 0x41), ("lit", 0x42)], lit1, [0])), name="no distance code, literals only"))
    items.append(item(stream(_dyn([("lit", 0x41), ("len", 257, 0), ("bits", 0, 1)], lit1, [0])), name="no distance code, a length symbol"))
    # a single literal/length code: only end-of-block, 1 bit; used and mis-used
    only_end = [0] * 256 + [1]
    items.append(item(stream(_dyn([], only_end, [0], cl_syms=R.rle_lengths(only_end + [0]))), name="only end-of-block"))
    items.append(item(stream(_dyn([("bits", 1, 1)], only_end, [0], end=False, cl_syms=R.rle_lengths(only_end + [0]))), name="only end-of-block, the unused code"))
    # HCLEN 4: only 16, 17, 18 and 0 exist, so every length is 0 and symbol 256 has no code
    cl4 = [0] * 19
    cl4[18], cl4[0] = 1, 1
    items.append(item(stream(_dyn([], [0] * 257, [0], end=False, cl_lens=cl4, hclen=4, cl_syms=[(18, 127), (18, 109)])), name="HCLEN 4"))
    # HCLEN 19 with repeats 16 / 17 / 18 at their smallest and largest counts, one of them crossing from the literal/length lengths into the
    # distance lengths: 253 x 8, 6 x 9, 0, 0, 0 | 0, 0, 0, 1, 10 x 0, 1, 11 x 0, 3 x 0  (lengths 3 and 4, distance symbols 3 and 14)
    litr = [8] * 253 + [9] * 6 + [0, 0, 0]
    distr = [0, 0, 0, 1] + [0] * 10 + [1] + [0] * 11 + [0] * 3
    syms_r = [(8, 0)] + [(16, 3)] * 41 + [(16, 0)] + [(8, 0)] * 3 + [(9, 0), (16, 2), (17, 3), (1, 0), (17, 7), (1, 0), (18, 0), (17, 0)]
    assert R.kraft(litr) == 32768 and R.kraft(distr) == 32768 and 1 + 41 * 6 + 3 + 3 == 253
    toks = [("lit", b) for b in PRELUDE[:200]] + [("match", 4, 4), ("match", 3, 150), ("lit", 0xFE), ("match", 4, 192), ("match", 3, 129), ("lit", 0xFD)]
    items.append(item(stream(_dyn(toks, litr, distr, cl_syms=syms_r)), name="repeats 16 / 17 / 18 at min and max, one across the boundary"))
    assert R.CL_FLAT[15] and items[-1]["want"][0] == R.OK                                          # (19 code-length lengths are written)
    # 18 at its largest count (138 zeros)
    lit18 = [1] + [0] * 138 + [2] + [0] * 116 + [2]
    syms18 = [(1, 0), (18, 127), (2, 0), (18, 105), (2, 0), (0, 0)]
    items.append(item(stream(_dyn([("lit", 0), ("lit", 139), ("lit", 0)], lit18, [0], cl_syms=syms18)), name="repeat 18 of 138"))
    # every malformed header, in a block that holds no symbol
    over = [1, 1, 1] + [0] * 253 + [2]
    inc = [2, 2] + [0] * 254 + [2]
    good = [1] + [0] * 255 + [1]
    bad = [("literal/length set over-subscribed", over, [0]), ("literal/length set incomplete", inc, [0]),
           ("distance set over-subscribed", good, [1, 1, 1]), ("distance set incomplete", good, [2, 2, 2]),
           ("distance set: one 2-bit code", good, [2])]
    for name, l, d in bad:
        items.append(item(stream(_dyn([], l, d, end=False)) + bytes(8), name=name))
        assert items[-1]["want"][0] == R.BAD, name
    items.append(item(stream(_dyn([("lit", 0)], good, [1, 1])), name="distance set of two 1-bit codes"))
    for c in IC.kats():                                                                           # ... the ones written down by hand
        if c["name"].startswith("dynamic:") and c["status"] == R.BAD:
            items.append(item(bytes.fromhex(c["src"]) + bytes(8), 64, c["name"]))
            assert items[-1]["want"][0] == R.BAD
    want = {"lengths 1..15": R.OK, "single distance code, used": R.OK, "single distance code, the unused code": R.BAD,
            "single distance code on symbol 3, distance 4 > produced": R.BAD, "no distance code, literals only": R.OK,
            "no distance code, a length symbol": R.BAD, "only end-of-block": R.OK, "only end-of-block, the unused code": R.BAD, "HCLEN 4": R.BAD,
            "repeat 18 of 138": R.OK, "distance set of two 1-bit codes": R.OK}
    for it in items:
        assert it["name"] not in want or it["want"][0] == want[it["name"]], (it["name"], it["want"][0])
        assert zlib_agrees(it), it["name"]
    check(items, "dynamic tables")


# ---------------------------------------------------------------------------------------------- block boundaries
def test_block_boundaries_at_every_bit_phase():
    """a fixed block of k nine-bit literals ends at bit 10 + 9k: the next block starts at every phase of a byte"""
    rng = random.Random(8)
    long_run = bytes(rng.randrange(256) for _ in range(65535))
    lit, dist = R.lens_for([("lit", 0x31), ("match", 5, 2)])
    items = []
    for k in range(8):
        head = lambda w, k=k: R.fixed_block(w, [("lit", 0x90 + j) for j in range(k)], False)
        tails = {
            "stored 0": lambda w: R.stored_block(w, b"", True, fill=1),
            "stored 1": lambda w: R.stored_block(w, b"Z", True),
            "stored 0 then fixed": lambda w: (R.stored_block(w, b"", False), R.fixed_block(w, [("lit", 0x33)], True)),
            "NLEN wrong": lambda w: R.stored_block(w, b"abc", True, nlen=0xFFFF),
            "type 3": lambda w: (w.put(1, 1), w.put(3, 2), w.put(0, 13)),
            "empty final fixed": lambda w: R.fixed_block(w, [], True),
            "dynamic": lambda w: R.dynamic_block(w, [("lit", 0x31), ("lit", 0x31), ("match", 5, 2)], True, lit, dist),
        }
        if k in (0, 3, 7):
            tails["stored 65535"] = lambda w: (R.stored_block(w, long_run, False), R.fixed_block(w, [("lit", 0x34)], True))
        for name, tail in tails.items():
            it = item(stream(head, tail), name="%s at phase %d" % (name, (10 + 9 * k) % 8))
            assert it["want"][0] == (R.BAD if name in ("NLEN wrong", "type 3") else R.OK) and zlib_agrees(it), it["name"]
            items.append(it)
    assert {(10 + 9 * k) % 8 for k in range(8)} == set(range(8))
    check(items, "block boundaries")


# ---------------------------------------------------------------------------------------------- prefixes, capacities, mutations
def test_every_prefix_of_a_stream_with_all_block_types():
    s, plain = IC.three_type_stream()
    assert 450 <= len(s) <= 800 and R.decode(s) == (R.OK, plain, len(s))
    items = [item(s[:cut], 2048, "prefix %d" % cut) for cut in range(len(s) + 1)]
    assert all(it["want"][0] == R.TRUNC for it in items[:-1]) and len({len(it["want"][1]) for it in items}) > 200
    check(items, "prefixes")


def test_every_capacity_of_a_small_stream():
    toks = [("lit", b) for b in b"capacity"] + [("match", 20, 3), ("lit", 0x2E), ("match", 3, 29)]
    lit, dist = R.lens_for(toks)
    s = stream(lambda w: R.stored_block(w, b"stored!", False), lambda w: R.dynamic_block(w, toks, False, lit, dist), lambda w: R.fixed_block(w, toks[:9], True))
    size = len(R.decode(s)[1])
    items = [item(s, cap, "cap %d" % cap) for cap in range(size + 2)]
    assert size == 7 + 32 + 28 and all(it["want"][0] == R.CAPACITY for it in items[:size]) and items[size]["want"][0] == items[size + 1]["want"][0] == R.OK
    check(items, "capacities")


def test_five_hundred_mutations():
    rng = random.Random(1951)
    bases = [IC.three_type_stream()[0], IC.raw_deflate(IC.text_like(1000, 21), 9), IC.raw_deflate(bytes(rng.randrange(3) for _ in range(900)), 6),
             IC.raw_deflate(IC.text_like(700, 22), 6, zlib.Z_FIXED)]
    items = []
    for i in range(500):
        m = bytearray(bases[i % len(bases)])
        for _ in range(1 + (i % 3 == 2)):
            k = rng.randrange(len(m))
            m[k] = m[k] ^ (1 << rng.randrange(8)) if rng.random() < 0.7 else rng.randrange(256)
        items.append(item(bytes(m), 1024, "mutation %d" % i))
    seen = {st: sum(it["want"][0] == st for it in items) for st in (R.OK, R.TRUNC, R.BAD, R.CAPACITY)}
    print(seen)
    assert seen[R.OK] >= 20 and seen[R.BAD] >= 20 and seen[R.CAPACITY] >= 20 and all(len(it["want"][1]) <= 1024 for it in items)
    check(items, "mutations")


# ---------------------------------------------------------------------------------------------- batches
_POOL = []


def pool():
    """a few dozen distinct valid streams from 0 bytes to 64 KiB, written by the standard library at every level and strategy"""
    if _POOL:
        return _POOL
    rng = random.Random(2025)
    noise = bytes(rng.randrange(256) for _ in range(20000))
    text = IC.text_like(65536, 31)
    mixed = b"".join(text[rng.randrange(60000):][:rng.randrange(3, 400)] + noise[rng.randrange(19000):][:rng.randrange(0, 40)] for _ in range(400))[:65536]
    k = 0
    for n in (0, 1, 2, 5, 17, 64, 100, 257, 1000, 2047, 2048, 2049, 4096, 9000, 20000, 40000, 65536):
        for data in (text[:n], mixed[:n]):
            _POOL.append(valid(data, IC.LEVELS[k % 4], IC.STRATEGIES[(k // 4) % 4]))
            k += 1
    _POOL.append(valid(bytes(50000), 9, name="zeros"))
    _POOL.append(valid(noise, 6, name="noise"))
    _POOL.append(valid(noise[:3000] * 12, 9, name="period 3000"))
    for it in _POOL[:12] + _POOL[-3:-2]:
        assert R.decode(it["src"]) == it["want"], it["name"]                                      # (the reference decoder agrees; once, on the small ones)
    return _POOL


@pytest.mark.parametrize("n", (1, 2, 65, 1500))
def test_batches_of_mixed_sizes(n):
    rng = random.Random(n)
    p = pool()
    items = [p[-1]] if n == 1 else [p[rng.randrange(len(p))] for _ in range(n)]
    if n >= 65:                                                                                    # ... some of them clipped, some cut
        for j in range(0, n, 7):
            it = items[j]
            items[j] = dict(it, cap=len(it["want"][1]) // 2, want=(R.CAPACITY, it["want"][1][:len(it["want"][1]) // 2], None)) if len(it["want"][1]) > 1 else it
    check(items, "batch of %d" % n)


def test_measure_the_size_and_limits():
    p = pool()
    c = ctx()
    items = [dict(it, cap=A.MEASURE_NO_BOUND) for it in p]
    streams, src, _ = pack(items)
    res = c.inflate_measure_batch(streams, src)
    for i, it in enumerate(items):
        compare("measure size %d (%s)" % (i, it["name"]), res[i], it, None)
    lim = [dict(it, cap=len(it["want"][1]) - 1 - k % 5, want=(R.CAPACITY, it["want"][1][:len(it["want"][1]) - 1 - k % 5], None)) for k, it in enumerate(p) if len(it["want"][1]) > 5]
    streams2, src2, _ = pack(lim)
    res2 = c.inflate_measure_batch(streams2, src2)
    for i, it in enumerate(lim):
        compare("measure limit %d (%s)" % (i, it["name"]), res2[i], it, None)
    assert all(res2[i].status == A.ST_OUTPUT_CAPACITY and res2[i].dst_len == lim[i]["cap"] for i in range(len(lim)))


# ---------------------------------------------------------------------------------------------- the file layers
def _file(fn, data, cap):
    lib = _lib.load()
    dst = np.full(max(cap, 1) + 16, GUARD, dtype=np.uint8)
    dl, su, st = C.c_size_t(12345), C.c_size_t(12345), C.c_int32(99)
    rc = getattr(lib, "alz_%s_decompress" % fn)(ctx().h, data, len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
    assert (dst[cap:] == GUARD).all()
    ml, mu, ms = C.c_size_t(12345), C.c_size_t(12345), C.c_int32(99)
    mrc = getattr(lib, "alz_%s_measure" % fn)(ctx().h, data, len(data), cap, C.byref(ml), C.byref(mu), C.byref(ms))
    if rc != A.E_CHECKSUM:                                                                         # measure takes the output checksums as correct
        assert (mrc, ms.value, ml.value, mu.value) == (rc, st.value, dl.value, su.value), (fn, rc, mrc)
    return rc, st.value, dl.value, su.value, dst[:dl.value].tobytes()


def test_file_layers():
    data = IC.text_like(5000, 41) + bytes(300) + IC.text_like(700, 42)
    n = len(data)
    zl, gz = F.ZLib(), F.GZip()
    for exact, variant, mode in MODES:
        select(exact, variant)
        try:
            # files the standard library wrote round-trip
            for level in (0, 1, 6, 9):
                z = zlib.compress(data, level)
                assert _file("zlib", z, n) == (0, A.ST_OK, n, len(z), data), (mode, level)
                g = gzip.compress(data, level, mtime=0)
                assert _file("gzip", g, n) == (0, A.ST_OK, n, len(g), data), (mode, level)
            z, g = zlib.compress(data, 6), gzip.compress(data, 6, mtime=0)
            assert zl.Decompress(z) == data and zl.last_src_used == len(z) and gz.Decompress(g) == data and gz.MeasureDecompressedSize(g) == n
            assert _file("zlib", z + b"trailing", n) == (0, A.ST_OK, n, len(z), data), mode             # *src_used = 2 + body + 4
            assert _file("zlib", zlib.compress(b"", 6), 0)[:4] == (0, A.ST_OK, 0, 8), mode
            assert _file("zlib", b"\x08\x1d" + z[2:], n)[:3] == (0, A.ST_OK, n), mode                    # CINFO 0 does not limit distances
            # a gzip file with FEXTRA + FNAME + FCOMMENT + FHCRC
            body, tail = g[10:-8], g[-8:]
            h = b"\x1f\x8b\x08\x1e" + g[4:10] + struct.pack("<H", 5) + b"extra" + b"name.bin\x00" + b"a comment\x00"
            full = h + struct.pack("<H", zlib.crc32(h) & 0xFFFF) + body + tail
            assert _file("gzip", full, n) == (0, A.ST_OK, n, len(full), data), mode
            assert gzip.decompress(full) == data
            bad_hcrc = h + struct.pack("<H", (zlib.crc32(h) & 0xFFFF) ^ 0x100) + body + tail
            assert _file("gzip", bad_hcrc, n)[0] == A.E_CHECKSUM, mode
            # two concatenated members; trailing garbage; both
            g2 = gzip.compress(b"second member " * 50, 9, mtime=0)
            both = data + b"second member " * 50
            assert _file("gzip", g + g2, len(both)) == (0, A.ST_OK, len(both), len(g + g2), both), mode
            assert _file("gzip", g + b"\x00garbage", n) == (0, A.ST_OK, n, len(g) + 8, data), mode
            assert _file("gzip", g + g2 + b"\x1f\x00", len(both)) == (0, A.ST_OK, len(both), len(g + g2) + 2, both), mode
            assert _file("gzip", g + g2, n + 10)[:3] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, n + 10), mode
            assert _file("gzip", g + g2[:7], n) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, n, len(g) + 7, data), mode   # a second member whose header is cut
            # a wrong Adler-32, a wrong CRC-32, a wrong ISIZE: the output is delivered
            wz = z[:-1] + bytes([z[-1] ^ 1])
            assert _file("zlib", wz, n) == (A.E_CHECKSUM, A.ST_OK, n, len(z), data), mode
            wc = g[:-8] + bytes([g[-8] ^ 1]) + g[-7:]
            assert _file("gzip", wc, n) == (A.E_CHECKSUM, A.ST_OK, n, len(g), data), mode
            wi = g[:-4] + struct.pack("<I", n + 1)
            assert _file("gzip", wi, n) == (A.E_CHECKSUM, A.ST_OK, n, len(g), data), mode
            with pytest.raises(F.InvalidDataException):
                zl.Decompress(wz)
            with pytest.raises(F.InvalidDataException):
                gz.Decompress(wi, n)
            # a cut trailer: INPUT_TRUNCATED with the output delivered
            for cut in (1, 3, 4):
                assert _file("zlib", z[:-cut], n) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, n, len(z) - cut, data), (mode, cut)
            for cut in (1, 4, 7, 8):
                assert _file("gzip", g[:-cut], n) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, n, len(g) - cut, data), (mode, cut)
            with pytest.raises(F.EndOfStreamException):
                zl.Decompress(z[:-2])
            # the body is cut; the capacity is one byte short; a bad body
            assert _file("zlib", z[:len(z) // 2], n)[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), mode
            r = _file("gzip", g, n - 1)
            assert r[:3] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, n - 1) and r[4] == data[:n - 1], mode
            with pytest.raises(BufferError):
                zl.Decompress(z, n - 1)
            assert _file("zlib", z[:2] + b"\x07" + z[3:], n)[:3] == (A.E_STREAM, A.ST_BAD_TOKEN, 0), mode    # block type 3
            # FDICT set; a header that is no header
            assert (0x78 * 256 + 0xBB) % 31 == 0 and _file("zlib", b"\x78\xbb" + z[2:], n)[0] == A.E_UNSUPPORTED, mode
            assert _file("zlib", g, n)[0] == A.E_FORMAT and _file("gzip", z, n)[0] == A.E_FORMAT, mode
            with pytest.raises(F.InvalidIdentifierException):
                gz.Decompress(z)
        finally:
            select(0, 0)
    with pytest.raises(NotImplementedError):
        zl.Compress(data)
