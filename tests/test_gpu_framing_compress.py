"""-m gpu: CRC-32C of byte ranges on the device (alz_crc32c_batch, alz_crc32c_batch_device) against the oracle, and LZ4 (frame, legacy) and
framed Snappy files WRITTEN in batches (alz_framing_compress_batch, CompressMany).  The file batch's contract is differential: for every
file what alz_container_compress on the same context returns for it alone with the same settings, block size and capacity, and the bytes it
writes; where that call fails only the code is comparable.  Sources sit at every residue mod 16, every destination lies between guard
bytes, every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib as O
import test_inflate_cpu as IC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 256
FILL = 0xA5
GAP = 64


# ---------------------------------------------------------------------------------------------------------------- CRC-32C
def table(ranges):
    t = (A.Stream * max(len(ranges), 1))()
    for i, (off, ln) in enumerate(ranges):
        t[i] = A.Stream(off, 0xDEAD0000 + i, ln, 0xBEEF, 0xF00D, 0xCAFE, 0xD00D, 77)          # everything but src_off / src_len is ignored
    return t


def both_forms(ranges, buf):
    """the batch through the host form and through the device form (the source between guard bytes): the values, identical in both"""
    c, t, n = ctx(), table(ranges), len(ranges)
    src = np.frombuffer(buf, dtype=np.uint8)
    host = c.crc32c_batch(t, src)[:n].copy()
    rng = np.random.default_rng(len(buf))
    image = np.concatenate([rng.integers(0, 256, GUARD, dtype=np.uint8), src, rng.integers(0, 256, GUARD, dtype=np.uint8)])
    d = c.malloc(image.nbytes)
    try:
        c.h2d(d, image)
        dev = c.crc32c_batch_device(t, C.c_void_p(d.value + GUARD), src.nbytes)[:n].copy()
        after = c.d2h(d, image.nbytes)
    finally:
        c.free(d)
    assert np.array_equal(after, image), "the device buffer changed"
    assert np.array_equal(host, dev), "host and device forms differ at %s" % np.nonzero(host != dev)[0][:5]
    return dev


_BUF = {}


def rand_bytes(n):
    if n not in _BUF:
        _BUF[n] = random.Random(n).randbytes(n)
    return _BUF[n]


def test_crc32c_every_length_at_every_offset_as_one_batch():
    buf = rand_bytes(200 + 16)
    ranges = [(off, ln) for ln in range(201) for off in range(16)]
    got = both_forms(ranges, buf)
    for (off, ln), g in zip(ranges, got):
        assert int(g) == O.crc32c(buf[off:off + ln]), (off, ln, hex(int(g)))
    assert int(got[0]) == 0                                                        # the empty range


def test_crc32c_lengths_around_the_chunk():
    lens = (32767, 32768, 32769, 65536, 65537, 98305)
    buf = rand_bytes(max(lens) + 16)
    ranges = [(off, ln) for ln in lens for off in (0, 1, 15)]
    got = both_forms(ranges, buf)
    for (off, ln), g in zip(ranges, got):
        assert int(g) == O.crc32c(buf[off:off + ln]), (off, ln, hex(int(g)))


def test_crc32c_one_large_range_at_an_odd_offset():
    n = (1 << 20) + 13
    buf = rand_bytes(n + 64)
    got = both_forms([(13, n)], buf)
    assert int(got[0]) == O.crc32c(buf[13:13 + n]), hex(int(got[0]))


def test_crc32c_mixed_batch_comes_back_in_input_order():
    rng = random.Random(300)
    buf = rand_bytes((1 << 20) + 4096)
    lens = (0, 1, 15, 16, 17, 1023, 1024, 5553, 32767, 32768, 32769, 65537)
    ranges = []
    for i in range(300):
        ln = rng.choice(lens)
        ranges.append((rng.randrange(0, len(buf) - ln + 1), ln))
        if i % 7 == 3:
            ranges[-1] = ranges[rng.randrange(len(ranges))]                                    # an identical range
        elif i % 7 == 5 and ranges[-2][1]:
            ranges[-1] = (ranges[-2][0] + ranges[-2][1] // 2, min(ln, len(buf) - ranges[-2][0] - ranges[-2][1] // 2))   # one that overlaps its neighbour
        elif i % 7 == 6:
            ranges[-1] = (ranges[-1][0], 0)                                                    # an empty one
    ranges[150] = (rng.randrange(1, 4096), 1 << 20)                                            # one 1 MiB range in the middle
    got = both_forms(ranges, buf)
    memo = {}
    for i, (r, g) in enumerate(zip(ranges, got)):
        if r not in memo:
            memo[r] = O.crc32c(buf[r[0]:r[0] + r[1]])
        assert int(g) == memo[r], (i, r, hex(int(g)))


def test_crc32c_check_value_and_arguments():
    c = ctx()
    nine = np.frombuffer(b"123456789", dtype=np.uint8)
    assert int(both_forms([(0, 9)], b"123456789" + bytes(7))[0]) == 0xE3069283
    assert int(c.crc32c_batch(table([(0, 9)]), nine)[0]) == 0xE3069283
    buf = np.frombuffer(rand_bytes(4096), dtype=np.uint8)
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    p = buf.ctypes.data_as(C.c_void_p)
    t = table([(0, 100), (4000, 96)])
    for fn in (c.lib.alz_crc32c_batch, c.lib.alz_crc32c_batch_device):
        assert fn(c.h, 0, None, 0, None, None) == 0                                            # n == 0
        assert fn(c.h, 2, p, 4095, t, out) == A.E_INVALID                                      # a range outside src_bytes
        assert fn(c.h, 2, p, 4096, None, out) == A.E_INVALID and fn(c.h, 2, p, 4096, t, None) == A.E_INVALID
    for fn in (c.lib.alz_checksum_batch, c.lib.alz_checksum_batch_device):
        assert fn(c.h, 2, 2, p, 4096, t, out) == A.E_INVALID                                   # not a kind of the checksum family
    assert list(out) == [7, 7, 7, 7]
    assert c.lib.alz_crc32c_batch(c.h, 2, p, 4096, t, out) == 0 and c.last_kernel_ms() > 0
    assert [out[0], out[1]] == [O.crc32c(bytes(buf[:100])), O.crc32c(bytes(buf[4000:4096]))]


# ---------------------------------------------------------------------------------------------------------------- the file batch
_FILES = None


def files():
    """[(container, aux0, raw bytes, name)]: every input as a frame of 64 KiB and of 256 KiB blocks, as a legacy file and as Snappy"""
    global _FILES
    if _FILES is None:
        inputs = [("text %d" % n, IC.text_like(n, 40 + i)) for i, n in enumerate((0, 1, 4, 5, 10, 65535, 65536, 65537, 65540, 65541, 3 * 65536 + 777))]
        inputs += [("random 70000", random.Random(7).randbytes(70000)), ("zeros 150000", bytes(150000)), ("text 200000", IC.text_like(200000, 11))]
        out = []
        for name, raw in inputs:
            out += [(A.C_LZ4_FRAME, 0x10000, raw, name + " frame 64K"), (A.C_LZ4_FRAME, 0x40000, raw, name + " frame 256K"),
                    (A.C_LZ4_LEGACY, 0, raw, name + " legacy"), (A.C_SNAPPY, 0, raw, name + " snappy")]
        pieces = [IC.text_like(65536, 90 + k) for k in range(4)]
        big = b"".join(pieces[k % 4] for k in range(65))[:(4 << 20) + 5]
        out.append((A.C_LZ4_FRAME, 0, big, "4 MiB + 5 frame default"))                          # two default blocks
        _FILES = out
    return _FILES


def bound(ct, n):
    lib = ctx().lib
    lib.alz_container_compress_bound.restype = C.c_size_t
    lib.alz_container_compress_bound.argtypes = [C.c_uint32, C.c_size_t]
    return int(lib.alz_container_compress_bound(ct, n))


_SINGLE = {}


def single(k, quality, cap=None):
    """alz_container_compress on file k alone, once per capacity: (rc, dst_len, the bytes written)"""
    ct, aux0, raw, _ = files()[k]
    cap = bound(ct, len(raw)) if cap is None else cap
    key = (k, quality, cap)
    if key not in _SINGLE:
        c = ctx()
        o = A.ContainerOptions()
        o.chunk_size = aux0
        st = A.Settings(quality, 0, 0, 0)
        dst = np.full(max(cap, 1), FILL, dtype=np.uint8)
        dl = C.c_size_t(0)
        c.lib.alz_container_compress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        rc = c.lib.alz_container_compress(c.h, ct, C.byref(o), C.byref(st), raw, len(raw), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl))
        _SINGLE[key] = (rc, int(dl.value) if rc == 0 else 0, dst[:dl.value].tobytes() if rc == 0 else b"")
    return _SINGLE[key]


def set_budget(nbytes):
    lib = ctx().lib
    lib.alz_debug_framing_compress_budget.argtypes = [C.c_void_p, C.c_uint64]
    lib.alz_debug_framing_compress_budget_get.restype = C.c_uint64
    assert lib.alz_debug_framing_compress_budget(ctx().h, nbytes) == 0
    return int(lib.alz_debug_framing_compress_budget_get())


def run_batch(quality, caps=None, aux0s=None):
    """all files in ONE call: sources at every residue mod 16, destinations between guard gaps.  -> [(rc, status, dst_len, src_used, bytes)]"""
    fs = files()
    tab = (A.Stream * len(fs))()
    src, so, do = bytearray(), 0, GAP
    for k, (ct, aux0, raw, _) in enumerate(fs):
        so = len(src) + ((k % 16) - len(src)) % 16
        src += bytes(so - len(src)) + raw
        cap = bound(ct, len(raw)) if caps is None or k not in caps else caps[k]
        tab[k] = A.Stream(so, do, len(raw), cap, 0xDEAD, aux0 if aux0s is None or k not in aux0s else aux0s[k], 0xBEEF, ct)   # decom_len and aux1 are ignored
        do += cap + GAP
    assert {int(t.src_off) % 16 for t in tab} == set(range(16))
    dst = np.full(do, FILL, dtype=np.uint8)
    dst, res = ctx().framing_compress_batch(tab, np.frombuffer(bytes(src) + bytes(1), dtype=np.uint8), do, dst=dst, quality=quality)
    out, inside = [], np.zeros(do, dtype=bool)
    for k, r in enumerate(res):
        a = int(tab[k].dst_off)
        inside[a:a + int(tab[k].dst_cap)] = True
        out.append((r.rc, r.status, r.dst_len, r.src_used, dst[a:a + r.dst_len].tobytes()))
    assert (dst[~inside] == FILL).all(), "a guard byte changed at %s" % np.nonzero((dst != FILL) & ~inside)[0][:5]
    return out


_BATCH = {}


def batch(quality):
    if quality not in _BATCH:
        _BATCH[quality] = run_batch(quality)
    return _BATCH[quality]


def same_as_single(got, k, quality, cap=None):
    rc, dl, data = single(k, quality, cap)
    name = files()[k][3]
    assert got[0] == rc and got[1] == A.ST_OK and got[2] == dl, (name, quality, got[:4], rc, dl)
    assert got[3] == (len(files()[k][2]) if rc == 0 else 0), (name, got[:4])
    if rc == 0 and got[4] != data:
        at = next(i for i in range(dl) if got[4][i] != data[i])
        raise AssertionError("%s at quality %d: the batch's file differs from the single file's at byte %d of %d" % (name, quality, at, dl))


@pytest.mark.parametrize("quality", (0, 8))
def test_batch_equals_the_single_file_call(quality):
    got = batch(quality)
    for k in range(len(files())):
        same_as_single(got[k], k, quality)
    by_name = {f[3]: got[k][0] for k, f in enumerate(files())}
    assert by_name["text 65537 frame 64K"] == A.E_INVALID and by_name["text 65540 frame 64K"] == A.E_INVALID   # a last block of 1 and of 4 bytes
    assert by_name["text 65541 frame 64K"] == 0 and by_name["text 65537 frame 256K"] == 0 and by_name["text 65537 snappy"] == 0
    assert by_name["text 1 frame 64K"] == A.E_INVALID and by_name["text 4 legacy"] == A.E_INVALID and by_name["text 5 legacy"] == 0
    assert sum(rc == 0 for rc in by_name.values()) >= len(by_name) - 16
    # stored blocks and chunks are among the cases: random bytes do not shrink
    k = next(i for i, f in enumerate(files()) if f[3] == "random 70000 frame 64K")
    assert got[k][4][7:11] == (0x10000 | 0x80000000).to_bytes(4, "little")
    k = next(i for i, f in enumerate(files()) if f[3] == "random 70000 snappy")
    assert got[k][4][10] == 1


@pytest.mark.parametrize("quality", (0, 8))
def test_every_file_decodes_back_to_its_input(quality):
    got, fs = batch(quality), files()
    ok = [k for k in range(len(fs)) if got[k][0] == 0]
    tab = (A.Stream * len(ok))()
    blob, do = bytearray(), 0
    for j, k in enumerate(ok):
        tab[j] = A.Stream(len(blob), do, len(got[k][4]), len(fs[k][2]), 0, 0, 0, fs[k][0])
        blob += got[k][4]
        do += len(fs[k][2])
    dst, res = ctx().framed_decode_batch(tab, np.frombuffer(bytes(blob) + bytes(1), dtype=np.uint8), do + 1)
    for j, k in enumerate(ok):
        raw = fs[k][2]
        if fs[k][0] == A.C_LZ4_LEGACY and not raw:
            # The legacy writer turns no input into the magic and the end flag (LZ4.cs:113-160), and the legacy reader wants a block size
            # behind the magic (ReadLZ4L, LZ4.cs:96-111): the single-file pair does not read this file back either.  It yields the 0 bytes.
            assert got[k][4] == bytes.fromhex("02214c18ff")
            assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0, 4), fs[k][3]
            continue
        assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == (0, 0, len(raw), len(got[k][4])), fs[k][3]
        assert dst[int(tab[j].dst_off):int(tab[j].dst_off) + len(raw)].tobytes() == raw, fs[k][3]


def test_capacities_are_judged_per_file():
    quality, fs = 8, files()
    idx = {f[3]: k for k, f in enumerate(fs)}
    a, b, c = idx["text 200000 frame 64K"], idx["zeros 150000 legacy"], idx["text 65541 snappy"]
    exact = single(a, quality)[1]
    caps = {a: exact - 1, b: 15, c: 9}
    got, whole = run_batch(quality, caps=caps), batch(quality)
    for k in range(len(fs)):
        if k in caps:
            same_as_single(got[k], k, quality, caps[k])
            assert got[k][0] == A.E_NOMEM, fs[k][3]
        else:
            assert got[k] == whole[k], fs[k][3]                                                # the neighbours are unchanged
    # ... and the exact capacity is enough
    fit = run_batch(quality, caps={a: exact})
    assert fit[a] == whole[a]


@pytest.mark.parametrize("budget", (256 << 10, 1))
def test_results_do_not_depend_on_the_grouping(budget):
    quality = 0
    whole = batch(quality)
    try:
        assert set_budget(budget) == budget
        got = run_batch(quality)
    finally:
        assert set_budget(0) == 2 << 30                                                        # 0 gives the default back
    for k, f in enumerate(files()):
        assert got[k] == whole[k], f[3]


def test_arguments():
    c = ctx()
    L = c.lib
    raw = np.frombuffer(IC.text_like(1000, 5), dtype=np.uint8)
    p = raw.ctypes.data_as(C.c_void_p)
    dst = np.full(8192, FILL, dtype=np.uint8)
    d = dst.ctypes.data_as(C.c_void_p)
    res = (A.FileResult * 3)()
    tab = (A.Stream * 3)(A.Stream(0, 0, 1000, 2048, 0, 0x10000, 0, A.C_LZ4_FRAME), A.Stream(0, 2048, 1000, 2048, 0, 0, 0, A.C_SNAPPY), A.Stream(0, 4096, 1000, 2048, 0, 0, 0, A.C_LZ4_LEGACY))
    assert L.alz_framing_compress_batch(c.h, None, 0, None, 0, None, None, 0, None) == 0       # n == 0
    assert L.alz_framing_compress_batch(c.h, None, 3, p, 1000, None, d, 8192, res) == A.E_INVALID
    assert L.alz_framing_compress_batch(c.h, None, 3, p, 1000, tab, d, 8192, None) == A.E_INVALID
    assert L.alz_framing_compress_batch(c.h, None, 3, p, 999, tab, d, 8192, res) == A.E_INVALID   # a range outside src_bytes
    assert L.alz_framing_compress_batch(c.h, None, 3, p, 1000, tab, d, 6143, res) == A.E_INVALID  # ... outside dst_bytes
    for fmt in (0, A.C_LZ4_FRAME + 1, 0xFFFFFFFF):
        bad = (A.Stream * 3)(*tab)
        bad[1].format = fmt
        assert L.alz_framing_compress_batch(c.h, None, 3, p, 1000, bad, d, 8192, res) == A.E_INVALID, fmt
    assert (dst == FILL).all()
    # NULL settings are quality 8; an aux0 the frame format does not have fails that file alone
    assert L.alz_framing_compress_batch(c.h, None, 3, p, 1000, tab, d, 8192, res) == 0
    first = [(r.rc, r.status, r.dst_len, r.src_used) for r in res]
    assert all(f[0] == 0 and f[3] == 1000 for f in first)
    dst2, res2 = c.framing_compress_batch(tab, raw, 8192, quality=8)
    assert [(r.rc, r.status, r.dst_len, r.src_used) for r in res2] == first and all(bytes(dst2[o:o + f[2]]) == bytes(dst[o:o + f[2]]) for o, f in zip((0, 2048, 4096), first))
    odd = (A.Stream * 3)(*tab)
    odd[0].aux0 = 0x20000
    odd[1].aux0 = 0x20000                                                                      # Snappy ignores it
    dst3, res3 = c.framing_compress_batch(odd, raw, 8192, quality=8)
    assert [(r.rc, r.status, r.dst_len, r.src_used) for r in res3] == [(A.E_INVALID, 0, 0, 0)] + first[1:]
    assert all(bytes(dst3[o:o + f[2]]) == bytes(dst[o:o + f[2]]) for o, f in zip((2048, 4096), first[1:]))


@pytest.mark.parametrize("cls,kw", ((F.LZ4, dict(BlockSize=0x10000)), (F.LZ4Legacy, {}), (F.Snappy, {})), ids=("LZ4", "LZ4Legacy", "Snappy"))
def test_compress_many_equals_compress(cls, kw):
    f = cls(**kw)
    datas = [IC.text_like(70000, 3), b"", IC.text_like(65537, 4), random.Random(9).randbytes(1000), IC.text_like(3, 5), bytes(200000)]
    many = f.CompressMany(datas)
    assert len(many) == len(datas) and f.CompressMany([]) == []
    raised = 0
    for x, got in zip(datas, many):
        try:
            want = f.Compress(x)
        except Exception as e:
            assert type(got) is type(e) and getattr(got, "code", None) == getattr(e, "code", None), (cls.__name__, len(x), got, e)
            raised += 1
            continue
        assert got == want, (cls.__name__, len(x))
    assert raised == {F.LZ4: 2, F.LZ4Legacy: 1, F.Snappy: 0}[cls]
    assert f.CompressMany(datas[:2], F.CompressionSettings.Fastest) == [f.Compress(x, F.CompressionSettings.Fastest) for x in datas[:2]]
