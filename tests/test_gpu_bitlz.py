"""-m gpu: CRILAYLA and ALLZ (alz_bitlz_*, alz_crilayla_*, alz_allz_*) on the device.  Every result field and every output byte against the
pure-Python restatement (tests/bitlz_ref.py) and, where one exists, the hand-assembled known answer (tests/golden/bitlz_kat.json).  Every
comparison is exact.  Every case runs under the exact, variant and default context modes (one kernel per format serves all three).
"""
import ctypes as C
import random

import numpy as np
import pytest

import bitlz_ref as R
import test_bitlz_cpu as BC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
FAMILIES = ((1, 0, "exact"), (0, 1, "variant"), (0, 0, "default"))       # (alz_ctx_set_exact_kernels, alz_ctx_set_kernel_variant)
GUARD = 0xA5
CRI, ALLZ = A.BITLZ_CRILAYLA, A.BITLZ_ALLZ
TRIPLES = ((0, 10, 1), (0, 0, 0), (2, 8, 3), (5, 14, 2), (7, 20, 9))
PRELUDE = bytes((131 * i * i + 7 * i + 3) % 251 + 1 for i in range(251))           # 251 non-zero bytes, no short period


# ---------------------------------------------------------------------------------------------- helpers
def cri_item(src, cap=None, name=""):
    """one CRILAYLA stream and the restatement's answer (computed once); cap None: exactly what it decodes to"""
    src = bytes(src)
    want = R.cri_decode(src, (1 << 24) if cap is None else cap)
    if cap is None:
        cap = want[2]
        want = R.cri_decode(src, cap)
    return dict(kind=CRI, src=src, cap=cap, decom=0xDEAD, aux0=0xBEEF, name=name, want=want)


def allz_item(src, decom, cap=None, params=(0, 10, 1), name=""):
    src = bytes(src)
    cap = decom if cap is None else cap
    return dict(kind=ALLZ, src=src, cap=cap, decom=decom, aux0=A.allz_aux0(*params), name=name, want=R.allz_decode(src, decom, cap, *params))


def allz_tokens_item(tokens, params=(0, 10, 1), name="", extra=0):
    """the stream of `tokens`, decoded to exactly what they produce (+ extra: decom_len beyond it)"""
    return allz_item(R.allz_assemble(tokens, *params), len(R.allz_expected(tokens)) + extra, None, params, name)


def pack(items, spread=False):
    """(streams, src array, dst_bytes).  spread: stream i's source sits at residue i mod 16; the END of a CRILAYLA span (dst_off + dst_cap) and
    the START of an ALLZ one sit at that residue too, 1..16 guard bytes behind the end of the neighbour's span"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        b = it["src"]
        mis = (i % 16) if spread else 0
        chunks.append(bytes(mis) + b + bytes((-(len(b) + mis)) % 16))
        if spread:
            do += 1
            anchor = do + it["cap"] if it["kind"] == CRI else do
            do += (i % 16 - anchor) % 16
        streams[i] = A.Stream(so + mis, do, len(b), it["cap"], it["decom"], it["aux0"], 0xF00D, it["kind"])
        so += len(chunks[-1])
        do = do + it["cap"] if spread else (do + it["cap"] + 15) // 16 * 16
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 16 + 64


def written(stream, it):
    """[a, b) of the destination that holds the stream's dst_len bytes"""
    n = it["want"][2]
    a = stream.dst_off + (it["cap"] - n if it["kind"] == CRI else 0)
    return a, a + n


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
    """the host form under every context mode"""
    streams, src, dst_bytes = pack(items, spread)
    for exact, variant, fam in FAMILIES:
        select(exact, variant)
        try:
            dst, res = ctx().bitlz_decode_batch(streams, src, dst_bytes)
        finally:
            select(0, 0)
        for i, it in enumerate(items):
            a, b = written(streams[i], it)
            compare("%s [%s] stream %d (%s)" % (what, fam, i, it["name"]), res[i], it, dst[a:b].tobytes())


def run_device(items, exact, variant):
    """device form on a destination pre-filled with guard bytes: (streams, whole destination, results, device ms)"""
    streams, src, dst_bytes = pack(items, True)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        c.memset(d_dst, GUARD, dst_bytes)
        select(exact, variant)
        try:
            res = c.bitlz_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
            ms = c.last_kernel_ms()
        finally:
            select(0, 0)
        return streams, c.d2h(d_dst, dst_bytes), res, ms
    finally:
        c.free(d_src)
        c.free(d_dst)


def cri_prelude(total):
    """tokens that produce `total` bytes of period 251"""
    toks = [("lit", b) for b in PRELUDE[:min(total, 251)]]
    if total > 251:
        toks.append(("match", 251, total - 251))
    return toks


def allz_prelude(total):
    assert total >= 254
    return [("run", PRELUDE), ("match", 251, total - 251)]


def cri_random_tokens(rng, nbytes, small=False):
    toks, produced = [], 0
    while produced < nbytes:
        if produced < 3 or rng.random() < (0.5 if small else 0.3):
            toks.append(("lit", rng.randrange(256))); produced += 1
            continue
        d = rng.choice([3, 4, 5, 7, 8, 15, 16, 17, 63, 64, 65, 100, 251, 1000, 4095, 4096, 4097, 5000, 8193, 8194])
        d = min(d, produced)
        L = rng.choice([3, 4, 5] if small else [3, 4, 5, 6, 12, 13, 16, 43, 44, 64, 65, 298, 299, 553, 554, 1023, 1024, 1025, 3000])
        toks.append(("match", d, L)); produced += L
    return toks


def allz_random_tokens(rng, nbytes, small=False):
    toks, produced = [("run", bytes(rng.randrange(256) for _ in range(rng.choice([1, 2, 5, 30]))))], 0
    produced = len(toks[0][1])
    while produced < nbytes:
        d = min(rng.choice([1, 2, 3, 4, 7, 8, 15, 16, 31, 63, 64, 65, 100, 300, 2000, 4095, 4096, 4097, 9000, 40000, 65535, 65536, 70000]), produced)
        L = rng.choice([3, 4, 5] if small else [3, 4, 5, 8, 15, 16, 17, 33, 64, 65, 200, 1023, 1024, 1025, 3000])
        toks.append(("match", d, L)); produced += L
        if rng.random() < 0.6:
            n = rng.choice([1, 2, 3] if small else [1, 2, 3, 7, 15, 16, 17, 60, 100, 511, 512, 513, 1100])
            toks.append(("run", bytes(rng.randrange(256) for _ in range(n)))); produced += n
    if toks[-1][0] == "run" and rng.random() < 0.5:                                    # (a run may end the stream; so may a match)
        toks.append(("match", 1, 3))
    return toks


_POOL = {}


def pool():
    """(small, big): a few dozen distinct streams of both kinds from 1 byte to 64 KiB, and one 1 MiB stream of each kind; answers computed once"""
    if _POOL:
        return _POOL["small"], _POOL["big"]
    rng = random.Random(2025)
    small = []
    for n in (1, 2, 3, 5, 17, 64, 100, 257, 1000, 4095, 4096, 4097, 9000, 20000, 30000, 65536):
        small.append(cri_item(R.cri_assemble(cri_random_tokens(rng, n), pad=n & 1), name="crilayla random %d" % n))
        small.append(allz_tokens_item(allz_random_tokens(rng, n), TRIPLES[n % 4], "allz random %d" % n))
    for n in (300, 5000, 30000):                                                       # many tokens per output byte
        small.append(cri_item(R.cri_assemble(cri_random_tokens(rng, n, small=True)), name="crilayla short tokens %d" % n))
        small.append(allz_tokens_item(allz_random_tokens(rng, n, small=True), name="allz short tokens %d" % n))
    small.append(cri_item(R.cri_assemble([("lit", 0x41)]), name="crilayla one literal"))
    small.append(allz_tokens_item([("run", b"Z")], name="allz one byte"))
    big = [cri_item(R.cri_assemble(cri_random_tokens(rng, 1 << 20) + [("match", 8194, 70000)]), name="crilayla 1 MiB"),
           allz_tokens_item(allz_random_tokens(rng, 1 << 20) + [("match", 300000, 70000)], name="allz 1 MiB")]
    assert all(it["want"][1] == R.OK for it in small + big) and min(it["want"][2] for it in big) >= 1 << 20
    _POOL["small"], _POOL["big"] = small, big
    return small, big


# ---------------------------------------------------------------------------------------------- known answers
def test_all_kats():
    items = []
    for c in BC.kats():
        if c["file"]:
            continue
        src = bytes.fromhex(c["src"])
        it = cri_item(src, c["cap"], c["name"]) if c["kind"] == "crilayla" else allz_item(src, c["decom_len"], c["cap"], tuple(c["params"]), c["name"])
        assert BC.ref_matches_kat(c, it["want"]), c["name"]
        items.append(it)
    assert len(items) >= 20
    check(items, "kat")
    check(items, "kat, spread", spread=True)


# ---------------------------------------------------------------------------------------------- CRILAYLA
CRI_LENGTHS = (3, 5, 6, 12, 13, 43, 44, 298, 299, 553, 554, 808, 809, 70000)
CRI_DISTANCES = (3, 4, 63, 64, 65, 4095, 4096, 4097, 8193, 8194)


def test_crilayla_every_vle_boundary_at_every_distance():
    """both sides of every step of the length code x both sides of the 4 KiB ring, of a wave and the largest distance, overlap included"""
    items = []
    for d in CRI_DISTANCES:
        for L in CRI_LENGTHS:
            toks = cri_prelude(8300) + [("lit", 0x31), ("match", d, L), ("lit", 0x32), ("match", d, 7), ("lit", 0x33)]
            items.append(cri_item(R.cri_assemble(toks), name="match(%d, %d)" % (d, L)))
    assert all(it["want"][1] == R.OK for it in items)
    check(items, "crilayla vle x distance", spread=True)


def test_crilayla_bit_phases_and_padding():
    kinds = {"lit": [("lit", 0x71)], "short": [("match", 4, 3)], "two fields": [("match", 9, 11)], "four fields": [("match", 30, 300)], "last": []}
    items = []
    for phase in range(8):
        for name, toks in kinds.items():
            for pad in (0, 1):
                t = cri_prelude(40) + [("lit", 0x70 + k) for k in range(phase)] + toks + ([("lit", 0x73)] if toks else [])
                items.append(cri_item(R.cri_assemble(t, pad=pad), name="%s at bit %d, padding %d" % (name, phase, pad)))
    assert all(it["want"][1] == R.OK for it in items)
    check(items, "crilayla bit phases")


def test_crilayla_distance_at_and_beyond_the_bytes_produced():
    """distance = produced is the last legal one; produced + 1 would read the neighbour's output, which lies right above the span"""
    items = []
    for p in (3, 4, 5, 63, 64, 65, 1000, 4096, 4097, 8193, 8194):
        for over in (0, 1):
            if p + over > 8194:
                continue
            toks = cri_prelude(p) + [("match", p + over, 9), ("lit", 0x55)]
            items.append(cri_item(R.cri_assemble(toks), name="distance %d at %d" % (p + over, p)))
            assert items[-1]["want"][1] == (R.BAD if over else R.OK) and items[-1]["cap"] == items[-1]["want"][2]
    items.append(cri_item(R.cri_assemble([("match", 3, 3)]), name="a match as the first token"))
    check(items, "crilayla distance = produced", spread=True)


def test_crilayla_every_front_cut_and_every_capacity():
    rng = random.Random(91)
    body = R.cri_assemble(cri_random_tokens(rng, 160, small=True))
    assert 70 <= len(body) <= 140, len(body)
    cuts = [cri_item(body[cut:], 4096, "front cut %d" % cut) for cut in range(len(body) + 1)]
    assert cuts[-1]["want"][1:] == (R.OK, 0, 0) and sum(it["want"][1] == R.TRUNC for it in cuts) >= 10
    check(cuts, "crilayla front cuts", spread=True)
    size = R.cri_decode(body, 4096)[2]
    check([cri_item(body, cap, "cap %d" % cap) for cap in range(size + 2)], "crilayla capacities", spread=True)


# ---------------------------------------------------------------------------------------------- ALLZ
def field_steps(s):
    """values on both sides of every prefix step of ReadALFlag(s), prefixes 0..3: 2^s - 1 | 2^s, 3 * 2^s - 1 | 3 * 2^s, ..."""
    out = []
    for k in range(1, 5):
        v = ((1 << k) - 1) << s
        out += [v - 1, v] if v else [v]
    return sorted(set(x for x in out if x >= 0))


def test_allz_every_prefix_step_of_every_field():
    items = []
    for params in TRIPLES:
        copy, dist, ln = params
        for v in field_steps(ln):                                                # run length v + 1
            toks = allz_prelude(300) + [("run", bytes((7 * i + v) % 256 for i in range(v + 1))), ("match", 1, 3)]
            items.append(allz_tokens_item(toks, params, "%s run %d" % (params, v + 1)))
        for v in field_steps(copy):                                              # match length v + 3
            toks = allz_prelude(300) + [("match", 7, v + 3), ("run", b"Z")]
            items.append(allz_tokens_item(toks, params, "%s length %d" % (params, v + 3)))
        for v in field_steps(dist):                                              # distance v + 1
            toks = allz_prelude(v + 300) + [("match", v + 1, 40), ("run", b"Z")]
            items.append(allz_tokens_item(toks, params, "%s distance %d" % (params, v + 1)))
    assert all(it["want"][1] == R.OK for it in items) and max(it["want"][2] for it in items) > 15 << 20
    check(items, "allz field steps")


def test_allz_runs_at_every_input_residue():
    """run lengths around a granule, a cache chunk and more than two of them; stream i's source sits at residue i mod 16"""
    items = []
    for n in (1, 15, 16, 17, 511, 512, 513, 1100, 5000):
        for r in range(16):
            toks = [("run", bytes((3 * i + n + r) % 256 for i in range(n))), ("match", min(n, 5), 9), ("run", bytes([r] * 3))]
            items.append(allz_tokens_item(toks, name="run %d at residue %d" % (n, r)))
    assert all(it["want"][1] == R.OK for it in items) and len(items) % 16 == 0
    check(items, "allz runs", spread=True)


def test_allz_bit_phases():
    """a no-run match is 13 bits with the default parameters: k of them in front put the token under test at every bit phase, so the flag
    byte runs out in front of a run, inside each of its fields and just behind it"""
    kinds = {"run 1": [("run", b"q"), ("match", 2, 3)], "run 20": [("run", bytes(range(20))), ("match", 2, 3)], "match": [("match", 5, 4)],
             "long fields": [("match", 70, 300)], "final run": [("run", b"xyz")], "run 600 + long match": [("run", bytes(i % 251 for i in range(600))), ("match", 500, 5000)]}
    items = []
    for phase in range(8):
        for name, toks in kinds.items():
            t = [("run", PRELUDE[:90])] + [("match", 3, 3)] * (phase + 1) + toks
            items.append(allz_tokens_item(t, name="%s behind %d matches" % (name, phase + 1)))
    assert all(it["want"][1] == R.OK for it in items)
    check(items, "allz bit phases")


def test_allz_distances_ring_readback_and_beyond():
    """320 KiB streams: both sides of a wave, of the LDS ring, of 64 KiB and of a 17-bit field; overlap and one match of 70000 bytes"""
    dists = (1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 0xFFFF, 0x10000, 0x1FFFF, 0x20000, 300000)
    items, all_toks = [], allz_prelude(320 << 10)
    for d in dists:
        tail = [("run", b"1"), ("match", d, 100), ("run", b"2"), ("match", d + 1, 1500), ("match", d, 3)]
        items.append(allz_tokens_item(allz_prelude(320 << 10) + tail, name="distance %d" % d))
        all_toks += tail
    items.append(allz_tokens_item(all_toks + [("match", 65, 70000), ("run", b"end")], name="all distances, then 70000 bytes at distance 65"))
    for d in (1, 2, 3, 63, 64, 65):
        for L in (d - 1, d, d + 1, 1000):
            if L >= 3:
                items.append(allz_tokens_item([("run", PRELUDE[:200]), ("match", d, L), ("run", b"!")], name="overlap d %d L %d" % (d, L)))
    assert all(it["want"][1] == R.OK for it in items)
    check(items, "allz distances", spread=True)


def test_allz_first_token_match_and_distance_at_the_bytes_produced():
    items = [allz_item(bytes.fromhex("0100"), 16, name="a match as the first token")]
    for params in TRIPLES[:4]:
        items.append(allz_item(R.allz_assemble([("match", 1, 3)], *params), 16, None, params, "%s a match as the first token" % (params,)))
    for p in (1, 2, 64, 65, 4096, 4097, 70000):
        for over in (0, 1):
            toks = [("run", (PRELUDE * (p // 251 + 1))[:p]), ("match", p + over, 9), ("run", b"Z")]
            items.append(allz_item(R.allz_assemble(toks), p + 10, name="distance %d at %d" % (p + over, p)))
            assert items[-1]["want"][1] == (R.BAD if over else R.OK)
    assert all(it["want"][1] == R.BAD for it in items[:5])
    check(items, "allz distance = produced", spread=True)


def test_allz_every_prefix_decom_len_and_capacity():
    rng = random.Random(92)
    toks = allz_random_tokens(rng, 220, small=True)
    body, size = R.allz_assemble(toks), len(R.allz_expected(toks))
    assert 60 <= len(body) <= 200, len(body)
    check([allz_item(body[:cut], size, name="prefix %d" % cut) for cut in range(len(body) + 1)], "allz prefixes", spread=True)
    check([allz_item(body, n, size + 1, name="decom_len %d" % n) for n in range(size + 2)], "allz decom_len", spread=True)
    check([allz_item(body, size, cap, name="cap %d" % cap) for cap in range(size + 2)], "allz capacities", spread=True)


def test_allz_wrapped_arithmetic():
    items = [allz_item(src, decom, cap, params, name) for name, src, decom, cap, params in BC.wrap_cases()]
    assert {it["want"][1] for it in items} >= {R.OK, R.BAD, R.TRUNC, R.MISMATCH, R.CAPACITY}
    check(items, "allz wraps")


# ---------------------------------------------------------------------------------------------- placement
def test_placement_guards_and_neighbours():
    """the device form on a destination full of guard bytes: 48 mixed streams, stream i's source at residue i mod 16, the END of a CRILAYLA span
    and the start of an ALLZ one at that residue; every byte outside the written ranges untouched -- below a CRILAYLA stream's dst_len bytes too"""
    rng = random.Random(5)
    items = []
    for k in range(48):
        n = rng.choice([1, 5, 40, 300, 2000, 6000, 12000])
        if (k // 3) % 2 == 0:
            body = R.cri_assemble(cri_random_tokens(rng, n), pad=k & 1)
            it = cri_item(body, name="crilayla %d" % k)
            if k % 3 == 1:
                it = cri_item(body, max(it["want"][2] - rng.randrange(1, 40), 0), it["name"] + " clipped")
            elif k % 3 == 2:
                it = cri_item(body, it["want"][2] + rng.randrange(1, 3000), it["name"] + " with room below")
        else:
            toks = allz_random_tokens(rng, n)
            it = allz_tokens_item(toks, TRIPLES[k % 4], "allz %d" % k)
            if k % 3 == 1:
                it = allz_item(it["src"], it["decom"], max(it["decom"] - rng.randrange(1, 40), 0), TRIPLES[k % 4], it["name"] + " clipped")
            elif k % 3 == 2:
                it = allz_item(it["src"], it["decom"] + 5, it["decom"] + 100, TRIPLES[k % 4], it["name"] + " truncated, room behind")
        items.append(it)
    assert {it["want"][1] for it in items} >= {R.OK, R.CAPACITY, R.TRUNC}
    host = None
    for exact, variant, fam in FAMILIES:
        streams, dst, res, ms = run_device(items, exact, variant)
        assert ms > 0
        mask = np.ones(dst.size, dtype=bool)
        for i, it in enumerate(items):
            s = streams[i]
            assert s.src_off % 16 == i % 16 and ((s.dst_off + s.dst_cap) if it["kind"] == CRI else s.dst_off) % 16 == i % 16
            a, b = written(s, it)
            compare("placement [%s] stream %d (%s)" % (fam, i, it["name"]), res[i], it, dst[a:b].tobytes())
            mask[a:b] = False
        assert (dst[mask] == GUARD).all(), "placement [%s]: %d guard bytes overwritten, first at %d" % (fam, int((dst[mask] != GUARD).sum()), int(np.nonzero(mask & (dst != GUARD))[0][0]))
        if host is None:                                                             # the device form gives what the host form gives
            host = ctx().bitlz_decode_batch(streams, pack(items, True)[1], dst.size)
        for i, it in enumerate(items):
            a, b = written(streams[i], it)
            assert (host[1][i].status, host[1][i].dst_len, host[1][i].src_used) == (res[i].status, res[i].dst_len, res[i].src_used)
            assert np.array_equal(host[0][a:b], dst[a:b])


def test_unknown_kind_is_refused():
    streams, src, dst_bytes = pack([cri_item(R.cri_assemble([("lit", 1)]))])
    streams[0].format = A.BITLZ_COUNT
    with pytest.raises(_lib.AlzError) as e:
        ctx().bitlz_decode_batch(streams, src, dst_bytes)
    assert e.value.code == A.E_INVALID


# ---------------------------------------------------------------------------------------------- batches
@pytest.mark.parametrize("n", (1, 2, 65, 1500))
def test_batches_of_mixed_sizes(n):
    rng = random.Random(n)
    small, big = pool()
    items = big[:n] if n <= 2 else [small[rng.randrange(len(small))] for _ in range(n - 2)] + big
    rng.shuffle(items)
    assert n <= 2 or {it["kind"] for it in items} == {CRI, ALLZ}
    check(items, "batch of %d" % n, spread=True)


# ---------------------------------------------------------------------------------------------- the file layers
def _decompress(fn, data, cap):
    dst = np.full(max(cap, 1) + 16, GUARD, dtype=np.uint8)
    dl, su, st = C.c_size_t(12345), C.c_size_t(12345), C.c_int32(99)
    rc = getattr(_lib.load(), fn)(ctx().h, data, len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
    assert (dst[cap:] == GUARD).all()
    return rc, st.value, dl.value, su.value, dst[:dl.value].tobytes()


def test_crilayla_file_layer():
    rng = random.Random(17)
    toks = cri_random_tokens(rng, 3000)
    body, plain = R.cri_assemble(toks), R.cri_expected(toks)[::-1]
    n, m = len(plain), len(body)
    hdr = bytes(rng.randrange(1, 256) for _ in range(0x100))
    cl = F.CRILAYLA()
    dec = lambda data, cap: _decompress("alz_crilayla_decompress", data, cap)
    for exact, variant, fam in FAMILIES:
        select(exact, variant)
        try:
            f = R.cri_file(body, n, hdr)
            assert cl.IsMatch(f) and cl.GetDecompressedSize(f) == n + 0x100
            assert dec(f, n + 0x100) == (0, A.ST_OK, n + 0x100, 16 + m + 0x100, hdr + plain), fam
            assert dec(f + b"trailing", n + 0x150)[:4] == (0, A.ST_OK, n + 0x100, 16 + m + 0x100), fam
            assert cl.Decompress(f) == hdr + plain and cl.last_src_used == len(f)
            assert R.cri_file_decode(f) == ("ok", R.OK, hdr + plain, len(f))
            # the body reaches 1, 255 and 256 bytes into the header region (:81): it wins there
            for k in (1, 255, 256):
                fk = R.cri_file(body, n - k, hdr)
                want = hdr[:0x100 - k] + plain
                assert R.cri_file_decode(fk)[2] == want
                assert dec(fk, n - k + 0x100) == (0, A.ST_OK, n - k + 0x100, len(fk), want), (fam, k)
            # fewer than 0x100 bytes behind the body: the missing ones are 0x00; none at all
            for have in (0, 1, 0xFF):
                fh = R.cri_file(body, n, hdr[:have])
                assert dec(fh, n + 0x100) == (0, A.ST_OK, n + 0x100, 16 + m + have, hdr[:have] + bytes(0x100 - have) + plain), (fam, have)
            # the body produces less than `size`: the bytes are delivered, zeros where nothing was written, then the error
            fs = R.cri_file(body, n + 9, hdr)
            assert dec(fs, n + 9 + 0x100) == (A.E_STREAM, A.ST_OUTPUT_SIZE_MISMATCH, n + 9 + 0x100, len(fs), hdr + bytes(9) + plain), fam
            with pytest.raises(F.DecompressedSizeException):
                cl.Decompress(fs)
            # format, size and capacity errors
            assert dec(f[:15], n + 0x100)[0] == A.E_FORMAT and dec(b"CRILAYLB" + f[8:], n + 0x100)[0] == A.E_FORMAT, fam
            with pytest.raises(F.InvalidIdentifierException):
                cl.Decompress(b"XRILAYLA" + f[8:], 10)
            assert dec(R.cri_file(body, 0x7FFFFF00, hdr), 64)[0] == A.E_UNSUPPORTED and dec(R.cri_file(body, 0xFFFFFFFF, hdr), 64)[0] == A.E_UNSUPPORTED, fam
            assert dec(f[:16 + m - 1], n + 0x100) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0, 16 + m - 1, b""), fam
            with pytest.raises(F.EndOfStreamException):
                cl.Decompress(f[:16 + m - 1])
            assert dec(f, n + 0xFF)[:3] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, 0), fam
            with pytest.raises(BufferError):
                cl.Decompress(f, n + 0xFF)
            # body errors pass through: a match beyond the bytes produced; a body that produces more than the span holds
            bad = R.cri_file(R.cri_assemble([("lit", 1), ("lit", 2), ("match", 3, 3)]), 2, hdr)
            assert dec(bad, 0x102)[:3] == (A.E_STREAM, A.ST_BAD_TOKEN, 0), fam
            with pytest.raises(ValueError):
                cl.Decompress(bad)
            assert dec(R.cri_file(body, n - 0x101, hdr), n)[:3] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, 0), fam
            # an empty body
            assert dec(R.cri_file(b"", 0, hdr), 0x100) == (0, A.ST_OK, 0x100, 16 + 0x100, hdr), fam
        finally:
            select(0, 0)
    for c in BC.kats():
        if c["file"] and c["kind"] == "crilayla":
            data = bytes.fromhex(c["src"])
            assert dec(data, c["dst_len"]) == (0, A.ST_OK, c["dst_len"], c["src_used"], bytes.fromhex(c["out"]))
    with pytest.raises(NotImplementedError):
        cl.Compress(plain)


def test_allz_file_layer():
    rng = random.Random(18)
    az = F.ALLZ()
    dec = lambda data, cap: _decompress("alz_allz_decompress", data, cap)
    for exact, variant, fam in FAMILIES:
        select(exact, variant)
        try:
            for params in TRIPLES[:4]:
                toks = allz_random_tokens(rng, 3000) + [("match", 2, 5)]                 # (the last token is longer than one byte)
                body, plain = R.allz_assemble(toks, *params), R.allz_expected(toks)
                n, m = len(plain), len(body)
                f = R.allz_file(body, n, *params)
                assert az.IsMatch(f) and az.GetDecompressedSize(f) == n
                assert dec(f, n) == (0, A.ST_OK, n, 12 + m, plain), (fam, params)
                assert dec(f + b"trailing", n + 7) == (0, A.ST_OK, n, 12 + m, plain), (fam, params)
                assert az.Decompress(f) == plain and az.last_src_used == 12 + m
            assert dec(f[:11], n)[0] == A.E_FORMAT and dec(b"ALLY" + f[4:], n)[0] == A.E_FORMAT, fam
            with pytest.raises(F.InvalidIdentifierException):
                az.Decompress(b"ALLY" + f[4:], 10)
            assert dec(R.allz_file(body, 0x80000000, *params), 64)[0] == A.E_UNSUPPORTED, fam
            assert dec(f[:12 + m - 1], n)[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED) and dec(f[:12 + m - 1], n)[3] == 12 + m - 1, fam
            with pytest.raises(F.EndOfStreamException):
                az.Decompress(f[:12 + m - 1])
            assert dec(f, n - 1)[:3] + (dec(f, n - 1)[4],) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, n - 1, plain[:n - 1]), fam
            with pytest.raises(BufferError):
                az.Decompress(f, n - 1)
            short = R.allz_file(body, n - 1, *params)                                  # the header's size ends inside the last token
            assert dec(short, n + 8)[:3] + (dec(short, n + 8)[4],) == (A.E_STREAM, A.ST_OUTPUT_SIZE_MISMATCH, n - 1, plain[:n - 1]), fam
            with pytest.raises(F.DecompressedSizeException):
                az.Decompress(short)
            assert dec(R.allz_file(bytes.fromhex("0100"), 16), 16)[:4] == (A.E_STREAM, A.ST_BAD_TOKEN, 0, 14), fam
            with pytest.raises(ValueError):
                az.Decompress(R.allz_file(bytes.fromhex("0100"), 16))
            assert dec(R.allz_file(b"", 0), 0) == (0, A.ST_OK, 0, 12, b""), fam
        finally:
            select(0, 0)
    for c in BC.kats():
        if c["file"] and c["kind"] == "allz":
            data = bytes.fromhex(c["src"])
            assert dec(data, c["dst_len"]) == (0, A.ST_OK, c["dst_len"], c["src_used"], bytes.fromhex(c["out"]))
    assert (az.LzCopyBits, az.LzDistanceBits, az.LzLengthBits) == R.ALLZ_DEFAULTS
    with pytest.raises(NotImplementedError):
        az.Compress(b"abc")
