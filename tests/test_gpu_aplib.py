"""-m gpu: aPLib (alz_aplib_*) on the device.  Both kernel families and the measure kernel, every result field and every output byte against the
pure-Python restatement (tests/aplib_ref.py) and, where one exists, the hand-assembled known answer (tests/golden/aplib_kat.json).  Every
comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import aplib_ref as R
import test_aplib_cpu as AC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from cases import prose_like
from gpu_common import ctx

pytestmark = pytest.mark.gpu
FAMILIES = ((1, 0, "exact"), (0, 1, "production"), (0, 0, "default"))       # (alz_ctx_set_exact_kernels, alz_ctx_set_kernel_variant)
GUARD = 0xA5


# ---------------------------------------------------------------------------------------------- helpers
def item(src, cap=None, name="", want=None):
    """one stream and the restatement's answer (computed once); cap None: what it decodes to, + 8"""
    src = bytes(src)
    if want is None:
        want = R.decode(src, (1 << 23) if cap is None else cap)
    if cap is None:
        cap = want[2] + 8
    return dict(src=src, cap=cap, name=name, want=want)


def pack(items, spread=False):
    """(streams, src array, dst_bytes).  spread: stream i sits at residue i mod 16 on both sides and its destination starts 1..16 bytes behind
    the end of its neighbour's capacity -- the gap is guard bytes"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        b = it["src"]
        mis = (i % 16) if spread else 0
        chunks.append(bytes(mis) + b + bytes((-(len(b) + mis)) % 16))
        if spread:
            do += 1
            do += (i % 16 - do) % 16
        streams[i] = A.Stream(so + mis, do, len(b), it["cap"], 0xDEAD, 0xBEEF, 0xF00D, 77)      # (decom_len, aux0, aux1, format are ignored)
        so += len(chunks[-1])
        do = do + it["cap"] if spread else (do + it["cap"] + 15) // 16 * 16
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 16 + 64


def compare(tag, r, it, got_bytes):
    out, status, dst_len, src_used = it["want"]
    assert (r.status, r.dst_len) == (status, dst_len), "%s: gpu status=%d len=%d used=%d | ref status=%d len=%d used=%s" % (
        tag, r.status, r.dst_len, r.src_used, status, dst_len, src_used)
    if src_used is not None:
        assert r.src_used == src_used, "%s: src_used gpu %d ref %d" % (tag, r.src_used, src_used)
    if got_bytes is not None and got_bytes != out:
        d = next(k for k in range(dst_len) if got_bytes[k] != out[k])
        raise AssertionError("%s: byte %d of %d differs (gpu %d, ref %d)" % (tag, d, dst_len, got_bytes[d], out[d]))


def select(exact, variant):
    ctx().set_exact_kernels(exact)
    ctx().set_kernel_variant(variant)


def check(items, what, spread=False):
    """host form under both families, then the measure kernel on the same streams"""
    streams, src, dst_bytes = pack(items, spread)
    for exact, variant, fam in FAMILIES:
        select(exact, variant)
        try:
            dst, res = ctx().aplib_decode_batch(streams, src, dst_bytes)
        finally:
            select(0, 0)
        for i, it in enumerate(items):
            a = streams[i].dst_off
            compare("%s [%s] stream %d (%s)" % (what, fam, i, it["name"]), res[i], it, dst[a:a + it["want"][2]].tobytes())
    res = ctx().aplib_measure_batch(streams, src)
    for i, it in enumerate(items):
        compare("%s [measure] stream %d (%s)" % (what, i, it["name"]), res[i], it, None)


def run_device(items, exact, variant, spread=True):
    """device form on a destination pre-filled with guard bytes: (streams, whole destination, results)"""
    streams, src, dst_bytes = pack(items, spread)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        c.memset(d_dst, GUARD, dst_bytes)
        select(exact, variant)
        try:
            res = c.aplib_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
            ms = c.last_kernel_ms()
        finally:
            select(0, 0)
        return streams, c.d2h(d_dst, dst_bytes), res, ms
    finally:
        c.free(d_src)
        c.free(d_dst)


PRELUDE = bytes((131 * i * i + 7 * i + 3) % 251 + 1 for i in range(251))           # 251 non-zero bytes, no short period


def prelude(total):
    """tokens that put `total` bytes of period 251 in front (PRELUDE[0] is the first byte): 250 literals and one long match"""
    toks = [("lit", b) for b in PRELUDE[1:]]
    if total > 251:
        toks.append(("match", 251, total - 251))
    return toks


def copy_tokens(d, L, lwm):
    """the token(s) that copy L bytes from distance d: a one-byte token, a short match, or a match (preceded by a literal when a match of this
    distance would read as a repeat)"""
    if L == 1 and 1 <= d <= 15:
        return [("one", d)]
    if L in (2, 3) and d <= 127:
        return [("short", d, L)]
    assert L - R.length_delta(d) >= 2, (d, L)
    return [("match", d, L)]


def random_tokens(rng, nbytes, small=False):
    """(first byte, tokens) of a valid stream of about nbytes: random tokens of every kind, distances beyond the start included (E2);
    small: short copies only (many tokens per output byte)"""
    toks, produced, lwm, last = [], 1, False, 0
    while produced < nbytes:
        k = rng.random()
        if k < 0.30:
            toks.append(("lit", rng.randrange(256))); produced += 1; lwm = False
        elif k < 0.40:
            toks.append(("one", rng.randrange(16))); produced += 1; lwm = False
        elif k < 0.55:
            d, L = rng.choice([1, 2, 3, 5, 17, 63, 64, 127]), rng.choice([2, 3])
            toks.append(("short", d, L)); produced += L; lwm, last = True, d
        elif k < 0.65 and not lwm:
            L = rng.choice([2, 3, 4] if small else [2, 3, 4, 9, 33, 100, 700])
            toks.append(("rep", L)); produced += L; lwm = True
        else:
            d = rng.choice([1, 2, 3, 4, 7, 8, 15, 16, 31, 64, 100, 0x7F, 0x80, 300, 0x4FF, 0x500, 2000, 2560, 2561, 4095, 4096, 4097, 9000, 0x7CFF, 0x7D00, 40000, 65535, 65536])
            if rng.random() < 0.5:
                d = min(d, produced)
            L = rng.choice([2, 3, 4, 5, 8] if small else [2, 3, 4, 5, 8, 15, 16, 17, 33, 64, 65, 200, 1023, 1024, 1025, 3000]) + R.length_delta(d)
            toks.append(("match", d, L)); produced += L; lwm, last = True, d
    toks.append(("end",))
    return rng.randrange(256), toks


_POOL = []


def pool():
    """a few dozen distinct streams from 1 byte to 64 KiB, each with its reference answer: greedy over prose and random token lists (seeded)"""
    if _POOL:
        return _POOL
    rng = random.Random(2024)
    for n in (1, 2, 3, 5, 17, 64, 100, 257, 1000, 4095, 4096, 4097, 9000, 20000):
        _POOL.append(item(R.greedy(prose_like(n, 100 + n)[:n]), name="greedy prose %d" % n))
    for n in (1, 2, 7, 63, 64, 65, 300, 1024, 2500, 5000, 5000, 12000, 12000, 30000, 65536, 65536):
        first, toks = random_tokens(rng, n)
        _POOL.append(item(R.assemble(first, toks), name="random tokens %d" % n))
    for n in (300, 5000, 30000):                                                          # many tokens per output byte: full queues
        first, toks = random_tokens(rng, n, small=True)
        _POOL.append(item(R.assemble(first, toks), name="random short tokens %d" % n))
    first, toks = R.greedy_tokens(prose_like(8192, 9))
    _POOL.append(item(R.assemble(first, toks[:-1] + [("match", 8192, 65536 - 8192), ("end",)]), name="greedy prose 8 KiB repeated to 64 KiB"))
    assert max(it["want"][2] for it in _POOL) >= 65536 and all(it["want"][1] == R.OK for it in _POOL)
    return _POOL


# ---------------------------------------------------------------------------------------------- known answers
def test_all_kats():
    items = []
    for c in AC.kats():
        src = bytes.fromhex(c["src"])
        ref = R.decode(src, c["cap"])
        assert ref[1:3] == (c["status"], c["dst_len"]) and AC.kat_matches(c, ref[0]) and (c["src_used"] is None or ref[3] == c["src_used"]), c["name"]
        items.append(item(src, c["cap"], c["name"], want=(ref[0], c["status"], c["dst_len"], c["src_used"])))
    check(items, "kat")


# ---------------------------------------------------------------------------------------------- token matrix
def test_one_byte_tokens_at_the_stream_start():
    """`one` with offsets 0..15 at produced = 1..16: offsets beyond the start read 0x00 (E2), not the neighbour's bytes"""
    items = []
    for p in range(1, 17):
        for off in range(16):
            toks = [("lit", b) for b in PRELUDE[1:p]] + [("one", off), ("lit", 0x99), ("end",)]
            items.append(item(R.assemble(PRELUDE[0], toks), name="one(%d) at %d" % (off, p)))
    assert any(it["want"][0][-2] == 0 for it in items) and any(it["want"][0][-2] != 0 for it in items)
    check(items, "one", spread=True)


def test_short_matches_and_length_delta_edges():
    items = []
    for d in (1, 2, 63, 64, 127):
        for L in (2, 3):
            for front in (1, 40, 300):                                                   # (fewer bytes than the distance: E2)
                toks = prelude(front)[:front - 1] + [("short", d, L), ("lit", 0x77), ("end",)]
                items.append(item(R.assemble(PRELUDE[0], toks), name="short(%d, %d) at %d" % (d, L, front)))
    for d in (0x7F, 0x80, 0x4FF, 0x500, 0x7CFF, 0x7D00):
        for lwm in (0, 1):
            for L in (2, 3, 9):
                L += R.length_delta(d)
                toks = prelude(0x7D40) + ([("short", 5, 2)] if lwm else [("lit", 0x31)]) + [("match", d, L), ("lit", 0x77), ("end",)]
                items.append(item(R.assemble(PRELUDE[0], toks), name="match(0x%X, %d) lwm %d" % (d, L, lwm)))
    check(items, "short / LengthDelta")


def test_distances_around_the_token_word_and_the_lds_window():
    """one 320 KiB stream per distance, and one with all of them: both sides of 0x1FFFF (the byte phase's distance field) and of the LDS ring"""
    dists = (2559, 2560, 2561, 4095, 4096, 4097, 0xFFFF, 0x10000, 0x1FFFF, 0x20000, 300000)
    items, all_toks = [], prelude(320 << 10)
    for d in dists:
        tail = [("lit", 0x31), ("match", d, 100), ("short", 7, 3), ("lit", 0x32), ("match", d + 1, 1500), ("lit", 0x33)]
        items.append(item(R.assemble(PRELUDE[0], prelude(320 << 10) + tail + [("end",)]), name="distance %d" % d))
        all_toks += tail
    items.append(item(R.assemble(PRELUDE[0], all_toks + [("end",)]), name="all distances"))
    # ... beyond the stream start (E2) at the same distances, in a short stream: the neighbour's output lies there
    for d in dists[6:]:
        items.append(item(R.assemble(PRELUDE[0], prelude(900) + [("match", d, 40), ("lit", 0x34), ("match", d, 2000), ("end",)]), name="distance %d beyond the start" % d))
    check(items, "distances", spread=True)


def test_repeats_and_gamma_values():
    items = []
    items.append(item(R.assemble(0x41, [("rep", 2), ("end",)]), name="rep first"))
    items.append(item(R.assemble(0x41, [("rep", 70000), ("lit", 1), ("end",)]), name="long rep first (distance 0 -> W -> zeros)"))
    items.append(item(R.assemble(PRELUDE[0], prelude(100) + [("short", 9, 2), ("lit", 0x51), ("rep", 7), ("one", 3), ("rep", 2), ("end",)]), name="rep after literal / one"))
    for g in (2, 3, 4, 7, 8, 255, 256, 65535, 70000):
        toks = prelude(600) + [("match", 300, g), ("lit", 0x52), ("rep", g), ("lit", 0x53), ("match", 0x600, g + 1), ("short", 3, 2), ("match", 0x600, g + 1), ("end",)]
        items.append(item(R.assemble(PRELUDE[0], toks), name="gamma %d" % g))
    for hi in (2, 3, 4, 7, 8, 255, 256):                                                  # ... as the distance's high part, with both biases
        d = hi << 8 | 0x21
        toks = prelude(70000) + [("lit", 0x54), ("match", d, 12), ("match", d + 256, 12), ("end",)]
        items.append(item(R.assemble(PRELUDE[0], toks), name="distance gamma %d" % hi))
    check(items, "rep / gamma")


def test_overlapping_matches():
    items = []
    for d in (1, 2, 3, 63, 64, 65):
        for L in (d - 1, d, d + 1, 1000, 70000):
            if L < 1 or (L == 1 and d > 15):
                continue
            for lwm in (0, 1):
                if L < 4 and lwm:
                    continue
                toks = prelude(200) + ([("short", 5, 2)] if lwm else [("lit", 0x61)]) + copy_tokens(d, L, lwm) + [("lit", 0x62), ("end",)]
                items.append(item(R.assemble(PRELUDE[0], toks), name="overlap d %d L %d lwm %d" % (d, L, lwm)))
    check(items, "overlap")


def test_every_token_kind_at_every_bit_phase():
    items = []
    kinds = {"lit": [("lit", 0x71)], "one": [("one", 3)], "zero": [("one", 0)], "short": [("short", 4, 3)], "match": [("match", 9, 11)],
             "far match": [("match", 0x1234, 300)], "rep": [("short", 6, 2), ("lit", 0x72), ("rep", 5)], "end": []}
    for phase in range(8):
        for name, toks in kinds.items():
            s = R.assemble(PRELUDE[0], prelude(40)[:39] + [("lit", 0x70 + k) for k in range(phase)] + toks + ([("lit", 0x73)] if toks else []) + [("end",)])
            items.append(item(s, name="%s at bit %d" % (name, phase)))
    check(items, "bit phases")


# ---------------------------------------------------------------------------------------------- errors
def test_every_prefix_and_every_capacity():
    rng = random.Random(90)
    first, toks = random_tokens(rng, 200, small=True)
    comp = R.assemble(first, toks)
    assert 70 <= len(comp) <= 130, len(comp)
    check([item(comp[:cut], 4096, "prefix %d" % cut) for cut in range(len(comp) + 1)], "prefixes", spread=True)
    size = R.decode(comp, 4096)[2]
    check([item(comp, cap, "cap %d" % cap) for cap in range(size + 2)], "capacities", spread=True)


def test_wrapped_distances_and_lengths():
    items = [
        item(R.assemble(0x55, [("gmatch", 0x00800003, 0x01, 2), ("end",)]), name="negative distance after the wrap"),
        item(R.assemble(0x55, [("lit", 1), ("gmatch", 3 + 0x2001, 0x00, 2), ("end",)]), name="distance W + 0x100"),
        item(R.assemble(0x55, [("lit", 0x66), ("gmatch", 3, 0x01, 0x80000000), ("gmatch", 2, 0x02, 2), ("end",)]), name="length <= 0 after the wrap"),
        item(R.assemble(0x55, [("lit", 0x66), ("short", 1, 2), ("lit", 3), ("gmatch", 2, 0, 0xFFFFFFFF), ("lit", 9), ("end",)]), name="repeat of length -1"),
        item(R.assemble(0x55, [("lit", 0x66), ("gmatch", (1 << 32) | 2, 0, 4), ("end",)]), name="gamma that wraps to 2 is a repeat"),
        item(R.assemble(0x55, [("gmatch", 0x00800003, 0x01, 1 << 20)])[:-1], name="input ends inside the length gamma of a bad distance"),
        item(b"", 16, name="empty input"),
        item(R.assemble(0x55, [("lit", 0x66), ("gmatch", 3, 0x01, 0x7FFFFFF0), ("end",)]), 5000, name="length 2^31 - 14 clipped by dst_cap"),
    ]
    assert [it["want"][1] for it in items] == [R.BAD, R.BAD, R.OK, R.OK, R.OK, R.TRUNC, R.TRUNC, R.CAPACITY]
    check(items, "wraps")


# ---------------------------------------------------------------------------------------------- placement
def test_placement_guards_and_neighbours():
    """the device form on a destination full of guard bytes: stream i at residue i mod 16 on both sides, every byte outside [dst_off, dst_off + dst_len)
    untouched, each output right behind its neighbour's (a source in front of the stream start must read 0x00, not the neighbour)"""
    rng = random.Random(5)
    items = []
    for k in range(48):
        first, toks = random_tokens(rng, rng.choice([1, 5, 40, 300, 2000, 6000]))
        it = item(R.assemble(first, toks), name="random %d" % k)
        if k % 3 == 1:
            it = item(it["src"], max(it["want"][2] - rng.randrange(1, 40), 0), it["name"] + " clipped")
        elif k % 3 == 2:
            it["cap"] = it["want"][2]                                                  # exactly what it needs
        items.append(it)
    host = None
    for exact, variant, fam in FAMILIES:
        streams, dst, res, ms = run_device(items, exact, variant)
        assert ms > 0
        mask = np.ones(dst.size, dtype=bool)
        for i, it in enumerate(items):
            a = streams[i].dst_off
            assert a % 16 == i % 16 and streams[i].src_off % 16 == i % 16
            compare("placement [%s] stream %d (%s)" % (fam, i, it["name"]), res[i], it, dst[a:a + it["want"][2]].tobytes())
            mask[a:a + it["want"][2]] = False
        assert (dst[mask] == GUARD).all(), "placement [%s]: %d guard bytes overwritten, first at %d" % (fam, int((dst[mask] != GUARD).sum()), int(np.nonzero(mask & (dst != GUARD))[0][0]))
        # the device form gives what the host form gives
        if host is None:
            host = ctx().aplib_decode_batch(streams, pack(items, True)[1], dst.size)
        for i, it in enumerate(items):
            a, n = streams[i].dst_off, it["want"][2]
            assert (host[1][i].status, host[1][i].dst_len) == (res[i].status, res[i].dst_len) and np.array_equal(host[0][a:a + n], dst[a:a + n])


# ---------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", (1, 2, 65, 1500))
def test_batches_of_mixed_sizes(n):
    rng = random.Random(n)
    p = pool()
    items = [p[-1]] if n == 1 else [p[rng.randrange(len(p))] for _ in range(n)]
    check(items, "batch of %d" % n, spread=True)


# ---------------------------------------------------------------------------------------------- measure
def test_measure_sizes_limits_and_device_form():
    p = pool()
    c = ctx()
    # "the size": dst_cap = 0xFFFFFF00
    items = [dict(it, cap=A.MEASURE_NO_BOUND) for it in p]
    streams, src, _ = pack(items, spread=True)
    res = c.aplib_measure_batch(streams, src)
    for i, it in enumerate(items):
        compare("measure size %d (%s)" % (i, it["name"]), res[i], it, None)
    # a limit below the size: OUTPUT_CAPACITY with dst_len = the limit; at the size: OK
    lim = [item(it["src"], max(it["want"][2] - 1 - k % 5, 0), it["name"]) for k, it in enumerate(p)] + [item(it["src"], it["want"][2], it["name"]) for it in p[:4]]
    streams2, src2, _ = pack(lim, spread=True)
    res2 = c.aplib_measure_batch(streams2, src2)
    for i, it in enumerate(lim):
        compare("measure limit %d (%s)" % (i, it["name"]), res2[i], it, None)
    assert all(res2[i].status == A.ST_OUTPUT_CAPACITY and res2[i].dst_len == lim[i]["cap"] for i in range(len(p)))
    # the device form: the same results, a device time, and nothing written -- the source buffer is what was uploaded
    d_src = c.malloc(src.nbytes)
    try:
        c.h2d(d_src, src)
        res3 = c.aplib_measure_batch_device(streams, d_src, src.nbytes)
        assert c.last_kernel_ms() > 0
        assert np.array_equal(c.d2h(d_src, src.nbytes), src)
    finally:
        c.free(d_src)
    for i in range(len(items)):
        assert (res3[i].status, res3[i].dst_len, res3[i].src_used) == (res[i].status, res[i].dst_len, res[i].src_used)


# ---------------------------------------------------------------------------------------------- the file layer
def _decompress(data, cap):
    lib = _lib.load()
    dst = np.full(max(cap, 1) + 16, GUARD, dtype=np.uint8)
    dl, su, st = C.c_size_t(12345), C.c_size_t(12345), C.c_int32(99)
    rc = lib.alz_aplib_decompress(ctx().h, data, len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
    assert (dst[cap:] == GUARD).all()
    return rc, st.value, dl.value, su.value, dst[:dl.value].tobytes()


def test_file_layer():
    data = prose_like(3000, 77)
    comp = R.greedy(data)
    n, m = len(data), len(comp)
    ap = F.APLib()
    for exact, variant, fam in FAMILIES:
        select(exact, variant)
        try:
            f24 = AC._file(24, comp, n)
            assert ap.IsMatch(f24) and ap.GetDecompressedSize(f24) == n
            assert _decompress(f24, n) == (0, A.ST_OK, n, 24 + m, data), fam
            assert ap.Decompress(f24) == data and ap.last_src_used == 24 + m
            # header size 32: eight bytes are skipped
            assert _decompress(AC._file(32, comp, n, pad=b"\xff" * 8), n + 5) == (0, A.ST_OK, n, 32 + m, data), fam
            # header size 20: 24 + (uint)(20 - 24) lands far beyond the end
            assert _decompress(AC._file(20, comp, n), n) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0, 24 + m, b""), fam
            with pytest.raises(F.EndOfStreamException):
                ap.Decompress(AC._file(20, comp, n), n)
            # the header's decoded size is wrong: the actual size comes back
            assert _decompress(AC._file(24, comp, n + 1), n + 8) == (A.E_STREAM, A.ST_OUTPUT_SIZE_MISMATCH, n, 24 + m, data), fam
            with pytest.raises(F.DecompressedSizeException):
                ap.Decompress(AC._file(24, comp, n - 1), n + 8)
            # a compressed-size field that is wrong is only traced by the reference
            wrong = bytearray(f24); wrong[8:12] = (m + 9).to_bytes(4, "little")
            assert _decompress(bytes(wrong), n)[:3] == (0, A.ST_OK, n), fam
            # truncated header: the magic and fewer than 24 bytes
            assert _decompress(f24[:23], n)[0] == A.E_FORMAT and _decompress(f24[:4], n)[0] == A.E_FORMAT, fam
            with pytest.raises(F.InvalidIdentifierException):
                ap.Decompress(f24[:23], n)
            # the body ends early
            assert _decompress(f24[:24 + m - 1], n)[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), fam
            # no magic: the whole input is a headerless body (fewer than four bytes too)
            assert _decompress(comp, n) == (0, A.ST_OK, n, m, data), fam
            assert ap.Decompress(comp) == data and ap.MeasureDecompressedSize(comp) == n
            tiny = R.assemble(0x41, [("end",)])
            assert len(tiny) == 3 and _decompress(tiny, 4) == (0, A.ST_OK, 1, 3, b"A"), fam
            assert _decompress(b"", 4)[:3] == (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0), fam
            # dst_cap one byte short
            assert _decompress(f24, n - 1)[:3] + (_decompress(f24, n - 1)[4],) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, n - 1, data[:n - 1]), fam
            with pytest.raises(BufferError):
                ap.Decompress(comp, n - 1)
        finally:
            select(0, 0)
    with pytest.raises(NotImplementedError):
        ap.Compress(data)


def test_single_literals_at_the_ring_seam():
    """aPLib is the one read-back configuration of the chunked copy phase with SINGLE literals: emit_steps stores them after the step's reads, into the ring and --
    for the first 32 slots -- into the mirror behind it (csrc/alz_emit_chunk.h:266-271).  A literal at ring offset 4096 k + {0, 1, 31, 32}, then a match
    whose source crosses that seam (near: it holds the literal) or the seam before it (read back), then matches of distance 4095 and 4096 with a literal directly
    behind them: that literal's ring slot is the one the last / the byte behind the last source byte had 4096 bytes ago."""
    items = []
    for k in (1, 2, 5):
        for off in (0, 1, 31, 32):
            P = 4096 * k + off
            for L in (8, 20):
                near, far = off + 9, 4096 + off + 9                                       # the source starts 8 bytes in front of a seam
                toks = prelude(P) + [("lit", 0xC3)] + copy_tokens(near, L + R.length_delta(near), False) + [("lit", 0xC4), ("match", far, L + R.length_delta(far)), ("lit", 0xC5)]
                for d in (4095, 4096):
                    toks += [("match", d, L + R.length_delta(d)), ("lit", 0xC6), ("lit", 0xC7)]
                it = item(R.assemble(PRELUDE[0], toks + [("end",)]), name="literal at %d, copies of %d" % (P, L))
                assert it["want"][1] == R.OK and it["want"][0][P] == 0xC3
                items.append(it)
    check(items, "literals at the seam", spread=True)
