"""-m gpu: Adler-32 and CRC-32 of byte ranges on the device (alz_checksum_batch, alz_checksum_batch_device) against the standard library's
zlib.adler32 / zlib.crc32.  Every batch goes through the host and the device entry point; the device buffer carries guard bytes in front of
and behind the source, downloaded and compared afterwards.  Every comparison is exact."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

from auroralib.compression_amd import _abi as A
from gpu_common import ctx

pytestmark = pytest.mark.gpu
KINDS = ((A.CK_ADLER32, zlib.adler32, "adler32"), (A.CK_CRC32, zlib.crc32, "crc32"))
GUARD = 256


def chunk_bytes():
    return int(ctx().lib.alz_debug_checksum_chunk(0))


def lengths():
    ck = chunk_bytes()
    assert ck % 1024 == 0 and 1024 <= ck <= 1 << 20
    return [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 5551, 5552, 5553, 65520, 65521, 65522, ck - 1, ck, ck + 1, 2 * ck + 1]


_DATA = {}


def data(name, n):
    """n bytes of one of the three data sets; all 0xFF gives the largest sums (the case that overflows an unreduced Adler accumulator)"""
    if (name, n) not in _DATA:
        _DATA[name, n] = {"random": lambda: random.Random(n).randbytes(n), "zeros": lambda: bytes(n), "ff": lambda: b"\xff" * n}[name]()
    return _DATA[name, n]


def table(ranges):
    t = (A.Stream * max(len(ranges), 1))()
    for i, (off, ln) in enumerate(ranges):
        t[i] = A.Stream(off, 0xDEAD0000 + i, ln, 0xBEEF, 0xF00D, 0xCAFE, 0xD00D, 77)          # everything but src_off / src_len is ignored
    return t


def both_forms(kind, ranges, buf):
    """the batch through the host form and through the device form (the source between guard bytes): the values, identical in both"""
    c, t, n = ctx(), table(ranges), len(ranges)
    src = np.frombuffer(buf, dtype=np.uint8)
    host = c._checksum(c.lib.alz_checksum_batch, kind, t, src.ctypes.data_as(C.c_void_p), src.nbytes)[:n].copy()
    rng = np.random.default_rng(len(buf))
    image = np.concatenate([rng.integers(0, 256, GUARD, dtype=np.uint8), src, rng.integers(0, 256, GUARD, dtype=np.uint8)])
    d = c.malloc(image.nbytes)
    try:
        c.h2d(d, image)
        dev = c._checksum(c.lib.alz_checksum_batch_device, kind, t, C.c_void_p(d.value + GUARD), src.nbytes)[:n].copy()
        after = c.d2h(d, image.nbytes)
    finally:
        c.free(d)
    assert np.array_equal(after, image), "the device buffer changed"
    assert np.array_equal(host, dev), "host and device forms differ at %s" % np.nonzero(host != dev)[0][:5]
    return dev


@pytest.mark.parametrize("name", ("random", "zeros", "ff"))
@pytest.mark.parametrize("kind,ref,kname", KINDS, ids=[k[2] for k in KINDS])
def test_every_length_at_every_offset(kind, ref, kname, name):
    ls = lengths()
    buf = data(name, max(ls) + 18)
    ranges = [(off, ln) for ln in ls for off in range(18)]
    got = both_forms(kind, ranges, buf)
    for (off, ln), g in zip(ranges, got):
        assert int(g) == ref(buf[off:off + ln]), (kname, name, off, ln, hex(int(g)))


@pytest.mark.parametrize("name", ("ff", "random"))
@pytest.mark.parametrize("kind,ref,kname", KINDS, ids=[k[2] for k in KINDS])
def test_one_large_range_at_an_odd_offset(kind, ref, kname, name):
    n = (5 << 20) + 17
    buf = data(name, n + 64)
    got = both_forms(kind, [(13, n)], buf)
    assert int(got[0]) == ref(buf[13:13 + n]), (kname, name, hex(int(got[0])))


@pytest.mark.parametrize("n", (1, 2, 65, 1500))
@pytest.mark.parametrize("kind,ref,kname", KINDS, ids=[k[2] for k in KINDS])
def test_mixed_batches_come_back_in_input_order(kind, ref, kname, n):
    rng = random.Random(n)
    big = 3 << 20
    buf = data("random", big + 4096)
    ls = lengths()
    ranges = []
    for i in range(n):
        ln = rng.choice(ls)
        ranges.append((rng.randrange(0, len(buf) - ln + 1), ln))
        if i % 7 == 3:
            ranges[-1] = ranges[rng.randrange(len(ranges))]                                    # an identical range
        elif i % 7 == 5 and ranges[-2][1]:
            ranges[-1] = (ranges[-2][0] + ranges[-2][1] // 2, min(ln, len(buf) - ranges[-2][0] - ranges[-2][1] // 2))   # one that overlaps its neighbour
    ranges[n // 2] = (rng.randrange(1, 4096), big)                                             # one 3 MiB range in the middle
    got = both_forms(kind, ranges, buf)
    memo = {}
    for i, (r, g) in enumerate(zip(ranges, got)):
        if r not in memo:
            memo[r] = ref(buf[r[0]:r[0] + r[1]])
        assert int(g) == memo[r], (kname, n, i, r, hex(int(g)))


def test_arguments():
    c = ctx()
    buf = np.frombuffer(data("random", 4096), dtype=np.uint8)
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    p = buf.ctypes.data_as(C.c_void_p)
    t = table([(0, 100), (4000, 96)])
    for fn in (c.lib.alz_checksum_batch, c.lib.alz_checksum_batch_device):
        assert fn(c.h, A.CK_CRC32, 0, None, 0, None, None) == 0                                # n == 0
        assert fn(c.h, 2, 2, p, 4096, t, out) == A.E_INVALID                                   # an unknown kind
        assert fn(c.h, A.CK_CRC32, 2, p, 4095, t, out) == A.E_INVALID                          # a range outside src_bytes
        assert fn(c.h, A.CK_CRC32, 2, p, 4096, None, out) == A.E_INVALID and fn(c.h, A.CK_CRC32, 2, p, 4096, t, None) == A.E_INVALID
    assert list(out) == [7, 7, 7, 7]
    assert c.lib.alz_checksum_batch(c.h, A.CK_CRC32, 2, p, 4096, t, out) == 0 and c.last_kernel_ms() > 0
    assert [out[0], out[1]] == [zlib.crc32(bytes(buf[:100])), zlib.crc32(bytes(buf[4000:4096]))]
    got = c.checksum_batch(A.CK_ADLER32, t, buf)
    assert [int(g) for g in got[:2]] == [zlib.adler32(bytes(buf[:100])), zlib.adler32(bytes(buf[4000:4096]))]
