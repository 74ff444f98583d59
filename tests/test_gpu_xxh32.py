"""-m gpu: XXH32 of byte ranges on the device (alz_xxh32_batch, alz_xxh32_batch_device) against the oracle's xxh32.  Every batch goes through
the host and the device entry point; the device buffer carries guard bytes in front of and behind the source, downloaded and compared
afterwards.  Every comparison is exact."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle_lib as O
from auroralib.compression_amd import _abi as A
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 256
UNROLL = 4                                          # ALZ_XXH32_UNROLL: stripes per loop iteration of the kernel as built (tests/test_framed_batch_cpu.py pins it)
SEEDS = (0, 0x9E3779B1)

_DATA = {}


def data(n):
    if n not in _DATA:
        _DATA[n] = random.Random(n).randbytes(n)
    return _DATA[n]


def table(ranges):
    t = (A.Stream * max(len(ranges), 1))()
    for i, (off, ln) in enumerate(ranges):
        t[i] = A.Stream(off, 0xDEAD0000 + i, ln, 0xBEEF, 0xF00D, 0xCAFE, 0xD00D, 77)          # everything but src_off / src_len is ignored
    return t


def both_forms(ranges, buf, seed):
    """the batch through the host form and through the device form (the source between guard bytes): the values, identical in both"""
    c, t, n = ctx(), table(ranges), len(ranges)
    src = np.frombuffer(buf, dtype=np.uint8)
    host = c.xxh32_batch(t, src, seed)[:n].copy()
    rng = np.random.default_rng(len(buf))
    image = np.concatenate([rng.integers(0, 256, GUARD, dtype=np.uint8), src, rng.integers(0, 256, GUARD, dtype=np.uint8)])
    d = c.malloc(image.nbytes)
    try:
        c.h2d(d, image)
        dev = c.xxh32_batch_device(t, C.c_void_p(d.value + GUARD), src.nbytes, seed)[:n].copy()
        after = c.d2h(d, image.nbytes)
    finally:
        c.free(d)
    assert np.array_equal(after, image), "the device buffer changed"
    assert np.array_equal(host, dev), "host and device forms differ at %s" % np.nonzero(host != dev)[0][:5]
    return dev


def check(ranges, buf, seed):
    got = both_forms(ranges, buf, seed)
    memo = {}
    for i, (r, g) in enumerate(zip(ranges, got)):
        if r not in memo:
            memo[r] = O.xxh32(buf[r[0]:r[0] + r[1]], seed)
        assert int(g) == memo[r], (i, r, hex(seed), hex(int(g)), hex(memo[r]))


def test_pinned_values():
    """XXH32("") and XXH32("abc") with seed 0 (held against the independent xxhash module when they were written down)"""
    assert O.xxh32(b"") == 0x02CC5D05 and O.xxh32(b"abc") == 0x32D153FF
    got = both_forms([(0, 0), (0, 3), (3, 0)], b"abc", 0)
    assert [int(g) for g in got] == [0x02CC5D05, 0x32D153FF, 0x02CC5D05]


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_every_length_at_every_offset(seed):
    """0 .. 80 bytes at start offsets 0 .. 15: the path below 16 bytes, the stripe loop, the dword tail, the byte tail, every alignment"""
    buf = data(80 + 16)
    check([(off, ln) for ln in range(81) for off in range(16)], buf, seed)


def test_lengths_around_the_unroll_boundary():
    step = 16 * UNROLL
    ls = sorted({k * step + d for k in (1, 2, 3, 8) for d in (-17, -16, -15, -1, 0, 1, 15, 16, 17)})
    buf = data(max(ls) + 16)
    check([(off, ln) for ln in ls for off in (0, 1, 2, 3, 4, 7, 13)], buf, 0)


@pytest.mark.parametrize("off", (13, 16))
def test_one_large_range(off):
    n = (1 << 20) + 13
    buf = data(n + 64)
    check([(off, n)], buf, 0)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("n", (1, 15, 16, 17, 1000))
def test_mixed_batches_come_back_in_input_order(n, seed):
    rng = random.Random(n)
    buf = data(300000)
    ranges = []
    for i in range(n):
        ln = rng.choice((0, rng.randrange(0, 16), rng.randrange(0, 300), rng.randrange(0, 5000), rng.randrange(0, 70001)))
        ranges.append((rng.randrange(0, len(buf) - ln + 1), ln))
        if i % 7 == 3:
            ranges[-1] = ranges[rng.randrange(len(ranges))]                                    # an identical range
        elif i % 7 == 5 and ranges[-2][1]:
            ranges[-1] = (ranges[-2][0] + ranges[-2][1] // 2, min(ln, len(buf) - ranges[-2][0] - ranges[-2][1] // 2))   # one that overlaps its neighbour
    ranges[n // 2] = (rng.randrange(1, 4096), 70000)
    ranges[-1] = (len(buf) - 37, 37)                                                           # one that ends with the buffer
    check(ranges, buf, seed)


def test_arguments():
    c = ctx()
    buf = np.frombuffer(data(4096), dtype=np.uint8)
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    p = buf.ctypes.data_as(C.c_void_p)
    t = table([(0, 100), (4000, 96)])
    for fn in (c.lib.alz_xxh32_batch, c.lib.alz_xxh32_batch_device):
        assert fn(c.h, 0, 0, None, 0, None, None) == 0                                         # n == 0
        assert fn(c.h, 0, 2, p, 4095, t, out) == A.E_INVALID                                   # a range outside src_bytes
        assert fn(c.h, 0, 2, p, 4096, None, out) == A.E_INVALID and fn(c.h, 0, 2, p, 4096, t, None) == A.E_INVALID
        assert fn(None, 0, 2, p, 4096, t, out) == A.E_INVALID
    assert list(out) == [7, 7, 7, 7]
    assert c.lib.alz_xxh32_batch(c.h, 5, 2, p, 4096, t, out) == 0 and c.last_kernel_ms() > 0
    assert [out[0], out[1]] == [O.xxh32(bytes(buf[:100]), 5), O.xxh32(bytes(buf[4000:4096]), 5)]
