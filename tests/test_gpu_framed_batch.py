"""-m gpu: LZ4 (frame, legacy) and framed Snappy files in batches (alz_framed_decode_batch, alz_framed_measure_batch, DecompressMany).  The
contract is differential: for every file the batch returns what the single-file call (alz_container_decompress / alz_container_measure) on
the same context returns for it alone with the same capacity, and delivers its bytes; where that call returns ALZ_E_FORMAT, ALZ_E_CHECKSUM
or ALZ_E_UNSUPPORTED only the code is comparable and the batch reports status OK and lengths of 0.  The generated files are held against the
byte-wise model of tests/framing_cases.py as well.  Sources sit at every residue mod 16, every destination lies between guard bytes, every
comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import framing_cases as FC
import oracle_lib as O
import test_inflate_cpu as IC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 0xA5
CT = {"lz4": A.C_LZ4_FRAME, "legacy": A.C_LZ4_LEGACY, "snappy": A.C_SNAPPY}
SMALL = 512 << 10                                   # cases whose model output is larger appear once, unmutated
DELIVERED = (0, A.E_STREAM)

_CORPUS = None


def corpus():
    """[dict(ct, data, name, expect, mids, ample)]: expect: the model's output of an unmutated generated file (None: a mutant -- the
    single-file call decides); ample: a capacity no smaller than what the file decodes to"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    out = []
    cases = FC.generated_cases(O.xxh32)
    for i, case in enumerate(cases):
        n = len(case.expect)
        out.append(dict(ct=CT[case.container], data=case.data, name=case.label, expect=case.expect, mids=case.mids, ample=n + 4096))
        if n <= SMALL:
            for mu in FC.mutants(case, FC.SEED * 7919 + i):
                out.append(dict(ct=CT[mu.container], data=mu.data, name=mu.label, expect=None, mids=case.mids, ample=n + (1 << 20)))
    text = IC.text_like(200000, 11)
    for cls, kw, nm in ((F.LZ4, dict(BlockSize=0x10000), "LZ4.Compress"), (F.LZ4Legacy, {}, "LZ4Legacy.Compress"), (F.Snappy, {}, "Snappy.Compress")):
        f = cls(**kw)
        out.append(dict(ct=f.container, data=f.Compress(text), name=nm, expect=text, mids=[0, 0x10000, 0x20000], ample=len(text) + 4096))
    # by hand: a Snappy chunk that decodes to more than it declares, with chunks behind it (the in-order path); twenty frames with content
    # checksums in one file (one round for all of them); a wrong content checksum in front of a truncated frame (the checksum decides)
    body = bytes([4, 9 << 2]) + b"0123456789"
    chunk = bytes([0, len(body) + 4, 0, 0]) + bytes(4) + body
    past = bytes([0xff, 6, 0, 0]) + b"sNaPpY" + chunk + bytes([1, 7, 0, 0]) + bytes(4) + b"abc" + chunk
    out.append(dict(ct=A.C_SNAPPY, data=past, name="snappy chunk past its declared size", expect=b"0123456789abc0123456789", mids=[0, 10, 13], ample=4096))
    rng = random.Random(20)
    parts = [rng.randbytes(rng.randrange(1, 3000)) for _ in range(20)]
    frames = [FC.lz4_frame([FC.lz4_seq(p[:len(p) // 2], 1, 9) + FC.lz4_seq(p[len(p) // 2:])], O.xxh32, flg=0x40 | 4, content=p[:len(p) // 2] + p[len(p) // 2 - 1:len(p) // 2] * 9 + p[len(p) // 2:])
              if len(p) >= 2 else FC.lz4_frame([FC.lz4_seq(p)], O.xxh32, flg=0x40 | 4, content=p) for p in parts]
    many = b"".join(frames)
    plain = b"".join(p[:len(p) // 2] + p[len(p) // 2 - 1:len(p) // 2] * 9 + p[len(p) // 2:] if len(p) >= 2 else p for p in parts)
    out.append(dict(ct=A.C_LZ4_FRAME, data=many, name="twenty frames with content checksums", expect=plain, mids=[0, len(plain) // 2], ample=len(plain) + 4096))
    wrong = bytearray(frames[0])
    wrong[-1] ^= 1
    out.append(dict(ct=A.C_LZ4_FRAME, data=bytes(wrong) + frames[1][:len(frames[1]) // 2], name="wrong content checksum in front of a truncated frame", expect=None, mids=[0], ample=1 << 16))
    _CORPUS = out
    return out


_SINGLE = {}


def single(k, cap, measure=False):
    """the single-file call on corpus item k, once per capacity: ((rc, status, dst_len, src_used), the bytes delivered)"""
    key = (k, cap, measure)
    if key in _SINGLE:
        return _SINGLE[key]
    it, c = corpus()[k], ctx()
    data = it["data"]
    dl, su, st = C.c_size_t(0), C.c_size_t(0), C.c_int32(0)
    if measure:
        rc = c.lib.alz_container_measure(c.h, it["ct"], None, data, len(data), cap, C.byref(dl), C.byref(su), C.byref(st))
        got = b""
    else:
        c.lib.alz_container_decompress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        dst = np.full(cap + 1, GUARD, dtype=np.uint8)
        rc = c.lib.alz_container_decompress(c.h, it["ct"], None, data, len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
        assert dl.value <= cap and dst[cap] == GUARD
        got = dst[:dl.value].tobytes() if rc in DELIVERED else b""
    _SINGLE[key] = ((rc, st.value, dl.value, su.value) if rc in DELIVERED else (rc, A.ST_OK, 0, 0), got)
    return _SINGLE[key]


def exact(k):
    """the capacity the file needs: what the single-file call delivers when it has room"""
    it = corpus()[k]
    return len(it["expect"]) if it["expect"] is not None else single(k, it["ample"])[0][2]


def pack(ks, caps):
    """(files, src, dst_bytes): file j is corpus item ks[j] with capacity caps[j]; sources at every residue mod 16, destinations between guard gaps"""
    items = corpus()
    files = (A.Stream * len(ks))()
    chunks, so, do = [], 0, 16
    for j, (k, cap) in enumerate(zip(ks, caps)):
        it, mis = items[k], j % 16
        chunks.append(bytes([0xEE]) * mis + it["data"])
        do += 1 + (j * 7) % 23
        files[j] = A.Stream(so + mis, do, len(it["data"]), cap, 0xDEAD, 0xBEEF, 0xF00D, it["ct"])
        so += len(chunks[-1])
        do += cap
    return files, np.frombuffer(b"".join(chunks) + bytes(1), dtype=np.uint8), do + 16


def refused():
    fn = ctx().lib.alz_debug_framed_batch_refused
    fn.restype = C.c_uint64
    return int(fn())


def check_decode(ks, caps):
    items = corpus()
    files, src, dst_bytes = pack(ks, caps)
    dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
    before = refused()
    out, res = ctx().framed_decode_batch(files, src, dst_bytes, dst=dst)
    assert out is dst
    assert refused() == before, "a decode did not confirm the measured sizes: the file went through the single-file layer"
    covered = np.zeros(dst_bytes, dtype=bool)
    seen = set()
    for j, (k, cap) in enumerate(zip(ks, caps)):
        it, r = items[k], res[j]
        want, want_bytes = single(k, cap)
        a = int(files[j].dst_off)
        assert (r.rc, r.status, r.dst_len, r.src_used) == want, (it["name"], j, cap, (r.rc, r.status, r.dst_len, r.src_used), want)
        if want[0] in DELIVERED:
            got = dst[a:a + r.dst_len].tobytes()
            assert got == want_bytes, (it["name"], j, cap, next(i for i in range(len(got)) if got[i] != want_bytes[i]))
        if it["expect"] is not None and cap >= len(it["expect"]):
            assert (r.rc, r.status, r.dst_len) == (0, A.ST_OK, len(it["expect"])) and want_bytes == it["expect"], (it["name"], j)
        covered[a:a + cap] = True
        seen.add((r.rc, r.status))
    assert (dst[~covered] == GUARD).all(), "bytes between two destinations were written"
    return seen


def test_every_file_of_the_corpus_in_one_batch_at_exact_capacities():
    ks = list(range(len(corpus())))
    assert len(ks) > 300 and {corpus()[k]["ct"] for k in ks} == set(CT.values())
    seen = check_decode(ks, [exact(k) for k in ks])
    for need in ((0, A.ST_OK), (A.E_FORMAT, A.ST_OK), (A.E_CHECKSUM, A.ST_OK), (A.E_STREAM, A.ST_INPUT_TRUNCATED), (A.E_STREAM, A.ST_OUTPUT_SIZE_MISMATCH)):
        assert need in seen, (need, seen)


def test_the_corpus_at_one_seeded_capacity_per_file():
    rng = random.Random(FC.SEED)
    ks = list(range(len(corpus())))
    caps = []
    for k in ks:
        n, mids = exact(k), corpus()[k]["mids"]
        caps.append(rng.choice((0, max(n - 1, 0), min(rng.choice(mids) if mids else 0, n), n + 100)))
    seen = check_decode(ks, caps)
    assert (A.E_STREAM, A.ST_OUTPUT_CAPACITY) in seen and (0, A.ST_OK) in seen, seen


def _first(pred):
    return next(k for k, it in enumerate(corpus()) if pred(it))


def test_batches_of_one_file():
    assert single(_first(lambda it: it["name"].startswith("wrong content checksum")), 1 << 16)[0][0] == A.E_CHECKSUM
    for k in (_first(lambda it: it["name"].startswith("snappy chunk past")), _first(lambda it: it["name"].startswith("twenty frames")), _first(lambda it: it["name"].startswith("wrong content checksum")),
              _first(lambda it: it["ct"] == A.C_LZ4_FRAME and it["expect"] is not None), _first(lambda it: it["ct"] == A.C_LZ4_LEGACY and it["expect"] is not None and len(it["expect"]) <= SMALL),
              _first(lambda it: it["ct"] == A.C_SNAPPY and it["expect"] is not None), _first(lambda it: it["expect"] is None), len(corpus()) - 1):
        check_decode([k], [exact(k)])


def test_a_shuffled_batch_of_1500_files():
    rng = random.Random(1500)
    small = [k for k in range(len(corpus())) if exact(k) <= (64 << 10)]
    assert len(small) >= 100 and {corpus()[k]["ct"] for k in small} >= {A.C_LZ4_FRAME, A.C_SNAPPY}     # (every legacy file of the corpus decodes to more)
    ks = [rng.choice(small) for _ in range(1500)]
    rng.shuffle(ks)
    check_decode(ks, [exact(k) for k in ks])


def test_the_content_checksum_is_in_the_loop():
    """a frame with a content checksum whose only block is stored: a flipped payload byte still 'decodes', only XXH32 of the output can tell"""
    c = ctx()
    payload = random.Random(4).randbytes(5000)
    good = FC.lz4_frame([payload], O.xxh32, flg=0x40 | 4, bd=0x40, content=payload, raw_flags=[True])
    at = good.index(payload[:16]) + 2500
    bad = good[:at] + bytes([good[at] ^ 0x40]) + good[at + 1:]
    files = (A.Stream * 2)(A.Stream(3, 7, len(good), 5000, 0, 0, 0, A.C_LZ4_FRAME), A.Stream(3 + len(good) + 5, 7 + 5000 + 9, len(bad), 5000, 0, 0, 0, A.C_LZ4_FRAME))
    src = np.frombuffer(bytes(3) + good + bytes(5) + bad + bytes(1), dtype=np.uint8)
    dst, res = c.framed_decode_batch(files, src, 7 + 5000 + 9 + 5000 + 3)
    assert (res[0].rc, res[0].status, res[0].dst_len, res[0].src_used) == (0, A.ST_OK, 5000, len(good)) and dst[7:5007].tobytes() == payload
    assert (res[1].rc, res[1].status, res[1].dst_len, res[1].src_used) == (A.E_CHECKSUM, A.ST_OK, 0, 0)
    c.lib.alz_container_decompress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    one = np.zeros(5000, dtype=np.uint8)
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert c.lib.alz_container_decompress(c.h, A.C_LZ4_FRAME, None, bad, len(bad), one.ctypes.data_as(C.c_void_p), 5000, C.byref(dl), C.byref(su), C.byref(st)) == A.E_CHECKSUM
    assert c.lib.alz_container_decompress(c.h, A.C_LZ4_FRAME, None, good, len(good), one.ctypes.data_as(C.c_void_p), 5000, C.byref(dl), C.byref(su), C.byref(st)) == 0


def test_measure_equals_the_single_file_measure():
    items = corpus()
    ks = list(range(len(items)))
    for limits in ([A.MEASURE_NO_BOUND] * len(ks), [exact(k) for k in ks], [100] * len(ks)):
        files, src, _ = pack(ks, [0] * len(ks))
        for j, lim in enumerate(limits):
            files[j].dst_cap = lim
        res = ctx().framed_measure_batch(files, src)
        for j, (k, lim) in enumerate(zip(ks, limits)):
            want = single(k, lim, measure=True)[0]
            assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == want, (items[k]["name"], lim, (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used), want)
            if items[k]["expect"] is not None and lim >= len(items[k]["expect"]):
                assert (res[j].rc, res[j].dst_len) == (0, len(items[k]["expect"])), items[k]["name"]
            if items[k]["expect"] is not None and lim == 100 and len(items[k]["expect"]) > 100:
                assert (res[j].rc, res[j].status) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY) and res[j].dst_len <= 100, items[k]["name"]
                if items[k]["ct"] != A.C_SNAPPY:                                   # (an LZ4 block is cut at the limit; a stored Snappy chunk that does not fit adds nothing)
                    assert res[j].dst_len == 100, items[k]["name"]


def test_arguments():
    c = ctx()
    k = _first(lambda it: it["ct"] == A.C_SNAPPY and it["expect"] is not None)
    it = corpus()[k]
    files, src, dst_bytes = pack([k], [exact(k)])
    dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
    res = (A.FileResult * 1)()
    sp, dp = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    assert c.lib.alz_framed_decode_batch(c.h, 0, None, 0, None, None, 0, None) == 0 and c.lib.alz_framed_measure_batch(c.h, 0, None, 0, None, None) == 0
    for fmt in (A.C_LZO, A.C_PRS, A.C_COUNT, 0xFFFFFFFF):
        files[0].format = fmt
        assert c.lib.alz_framed_decode_batch(c.h, 1, sp, src.nbytes, files, dp, dst_bytes, res) == A.E_INVALID    # not a container of this layer
        assert c.lib.alz_framed_measure_batch(c.h, 1, sp, src.nbytes, files, res) == A.E_INVALID
    files[0].format = it["ct"]
    assert c.lib.alz_framed_decode_batch(c.h, 1, sp, len(it["data"]) - 1, files, dp, dst_bytes, res) == A.E_INVALID     # the file outside src_bytes
    assert c.lib.alz_framed_measure_batch(c.h, 1, sp, len(it["data"]) - 1, files, res) == A.E_INVALID
    assert c.lib.alz_framed_decode_batch(c.h, 1, sp, src.nbytes, files, dp, int(files[0].dst_off) + int(files[0].dst_cap) - 1, res) == A.E_INVALID   # the slot outside dst_bytes
    assert c.lib.alz_framed_decode_batch(c.h, 1, sp, src.nbytes, None, dp, dst_bytes, res) == A.E_INVALID
    assert c.lib.alz_framed_decode_batch(c.h, 1, sp, src.nbytes, files, dp, dst_bytes, None) == A.E_INVALID
    assert c.lib.alz_framed_measure_batch(c.h, 1, sp, src.nbytes, None, res) == A.E_INVALID and c.lib.alz_framed_measure_batch(c.h, 1, sp, src.nbytes, files, None) == A.E_INVALID
    assert (dst == GUARD).all()


def test_decompress_many_against_a_loop_of_decompress():
    kinds, successes = set(), 0
    for cls, ct in ((F.LZ4, A.C_LZ4_FRAME), (F.LZ4Legacy, A.C_LZ4_LEGACY), (F.Snappy, A.C_SNAPPY)):
        items = [it for k, it in enumerate(corpus()) if it["ct"] == ct and exact(k) <= SMALL]
        assert sum(it["expect"] is not None for it in items) >= 2 and sum(it["expect"] is None for it in items) >= 10, cls
        f = cls()
        got = f.DecompressMany([it["data"] for it in items])
        assert len(got) == len(items) and f.DecompressMany([]) == []
        for it, g in zip(items, got):
            try:
                want = f.Decompress(it["data"])
            except Exception as e:
                want = e
            if isinstance(want, bytes):
                assert g == want and (it["expect"] is None or g == it["expect"]), (cls, it["name"], g if not isinstance(g, bytes) else len(g))
                successes += 1
            else:
                assert it["expect"] is None and type(g) is type(want), (cls, it["name"], g if not isinstance(g, bytes) else len(g), want)
                kinds.add(type(want))
    assert successes and {F.InvalidDataException, F.EndOfStreamException} <= kinds, kinds
