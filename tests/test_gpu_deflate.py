"""-m gpu: the DEFLATE encoder (alz_deflate_*) on the device.  Every stream it writes is held against three readers -- the standard
library's zlib (window bits -15: eof, nothing left over, the input back), alz_inflate_decode_batch on the GPU (OK, src_used == the
encoder's dst_len, the bytes) and the token walker of tests/deflate_walk.py (distances <= 32 768 and <= the position, lengths 3..258,
stored LEN <= 65 535).  Every batch is packed as tests/test_gpu_inflate.py packs (residue i mod 16 on both sides, guard bytes between
the slots) and runs through the host form and the device form in all three context modes with byte-identical outputs; with
ALZ_DEFLATE_FIXED no dynamic block appears and the default is never larger.  Every comparison is exact."""
import ctypes as C
import gzip
import random
import zlib

import numpy as np
import pytest

import deflate_walk as W
import test_gpu_inflate as TG
import test_inflate_cpu as IC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 0xA5
LEVELS = (0, 1, 6, 9)


def lib():
    return _lib.load()


def B():
    return lib().alz_deflate_block_bytes()


def bound(n):
    return lib().alz_deflate_bound(n)


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


def encode(datas, level, flags=0, caps=None, what=""):
    """the batch through both forms in all three modes: identical results and bytes everywhere, guards and source untouched -> (results, outputs)"""
    items = [dict(src=bytes(d), cap=bound(len(d)) if caps is None else caps[i]) for i, d in enumerate(datas)]
    streams, src, dst_bytes = TG.pack(items)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    first = None
    try:
        c.h2d(d_src, src)
        for exact, variant, mode in TG.MODES:
            TG.select(exact, variant)
            try:
                h_dst, h_res = c.deflate_encode_batch(streams, src, dst_bytes, level, flags, dst=np.full(dst_bytes, GUARD, dtype=np.uint8))
                c.memset(d_dst, GUARD, dst_bytes)
                d_res = c.deflate_encode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes, level, flags)
                assert c.last_kernel_ms() > 0
                dst = c.d2h(d_dst, dst_bytes)
            finally:
                TG.select(0, 0)
            res, outs = [], []
            mask = np.ones(dst.size, dtype=bool)
            for i, it in enumerate(items):
                tag = "%s level %d flags %d [%s] stream %d (%d bytes)" % (what, level, flags, mode, i, len(it["src"]))
                a, r, hr = streams[i].dst_off, d_res[i], h_res[i]
                assert a % 16 == i % 16 and streams[i].src_off % 16 == i % 16
                assert (r.status, r.dst_len, r.src_used) == (hr.status, hr.dst_len, hr.src_used), tag
                assert r.status in (A.ST_OK, A.ST_OUTPUT_CAPACITY), tag
                if r.status == A.ST_OK:
                    assert r.src_used == len(it["src"]) and r.dst_len <= it["cap"], tag
                else:
                    assert r.dst_len == 0, tag
                outs.append(dst[a:a + r.dst_len].tobytes())
                assert h_dst[a:a + r.dst_len].tobytes() == outs[-1], tag + ": host and device forms differ"
                res.append((r.status, r.dst_len))
                mask[a:a + r.dst_len] = False
            assert (dst[mask] == GUARD).all() and (h_dst[mask] == GUARD).all(), "%s [%s]: guard bytes overwritten" % (what, mode)
            if first is None:
                first = (res, outs)
            assert (res, outs) == first, "%s [%s]: the context mode changes the output" % (what, mode)
        assert np.array_equal(c.d2h(d_src, src.nbytes), src)
    finally:
        c.free(d_src)
        c.free(d_dst)
    return first


def walk_check(data, out, level, flags, tag):
    blocks, used = W.walk(out)
    assert used == len(out), tag
    pos = 0
    for b in blocks:
        assert b["start"] == pos
        if b["type"] == W.STORED:
            assert b["stored"] <= 65535, tag
            pos += b["stored"]
            continue
        assert level > 0, tag + ": level 0 writes stored blocks only"
        assert not (flags & A.DEFLATE_FIXED and b["type"] == W.DYNAMIC), tag + ": a dynamic block with ALZ_DEFLATE_FIXED"
        for t in b["tokens"]:
            if t[0] == "lit":
                pos += 1
            else:
                assert 3 <= t[1] <= 258 and 1 <= t[2] <= 32768 and t[2] <= pos, (tag, t, pos)
                pos += t[1]
    assert pos == len(data), tag
    return blocks


def read_back(datas, outs, level, flags, what, walk=True):
    """the three readers; returns the walker's blocks per stream"""
    for i, (d, o) in enumerate(zip(datas, outs)):
        z = zlib.decompressobj(-15)
        assert z.decompress(o) == bytes(d) and z.eof and z.unused_data == b"", "%s level %d flags %d stream %d: zlib" % (what, level, flags, i)
    items = [dict(src=o, cap=len(d) + 8) for d, o in zip(datas, outs)]
    streams, src, dst_bytes = TG.pack(items)
    dst, res = ctx().inflate_decode_batch(streams, src, dst_bytes)
    for i, (d, o) in enumerate(zip(datas, outs)):
        a = streams[i].dst_off
        assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(d), len(o)), "%s level %d flags %d stream %d: alz_inflate" % (what, level, flags, i)
        assert dst[a:a + len(d)].tobytes() == bytes(d)
    return [walk_check(d, o, level, flags, "%s level %d flags %d stream %d" % (what, level, flags, i)) for i, (d, o) in enumerate(zip(datas, outs))] if walk else None


def round_trip(datas, levels, what, walk=True):
    """default and fixed-only at every level: all OK within the bound, read back by the three readers, the default never larger"""
    got = {}
    for level in levels:
        sizes = {}
        for flags in (0, A.DEFLATE_FIXED):
            res, outs = encode(datas, level, flags, what=what)
            for i, d in enumerate(datas):
                assert res[i][0] == A.ST_OK and len(outs[i]) <= bound(len(d)) <= len(d) + (len(d) >> 10) + 64, (what, level, flags, i)
            got[(level, flags)] = (outs, read_back(datas, outs, level, flags, what, walk))
            sizes[flags] = [len(o) for o in outs]
        assert all(a <= b for a, b in zip(sizes[0], sizes[A.DEFLATE_FIXED])), "%s level %d: the default is larger than fixed-only" % (what, level)
    return got


# ---------------------------------------------------------------------------------------------- shapes
def test_sizes():
    lens = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259)
    datas = [IC.text_like(n, n) for n in lens] + [rnd(n, n) for n in lens]
    got = round_trip(datas, LEVELS, "sizes")
    for level in LEVELS:
        empty = got[(level, 0)][0][0]
        blocks, _ = W.walk(empty)
        assert len(blocks) == 1 and blocks[0]["final"] == 1, "empty input: one final block"


def test_runs():
    datas = [b"r" * n for n in (3, 4, 258, 259, 260, 261, 516, 517, 70000)] + [b"ab" * 40000]
    got = round_trip(datas, (1, 6, 9), "runs")
    for level in (1, 6, 9):
        outs, walks = got[(level, 0)]
        assert len(outs[8]) < 700 and len(outs[9]) < 800, "a run of 70 000 bytes takes %d, the period takes %d" % (len(outs[8]), len(outs[9]))
        m = [t for b in walks[2] for t in b["tokens"] if t[0] == "match"]
        assert m and m[0][2] == 1, "a run of 258: distance 1"
        assert any(t[1] == 258 for b in walks[8] for t in b["tokens"] if t[0] == "match")


def test_every_length():
    # (random over 64 values: 300 bytes drawn from all 256 with ONE short match are smallest as a stored block, by the very rule that a block
    # takes its smallest form, and a stored block shows the walker no token)
    seed = bytes(b & 63 for b in rnd(300, 5))
    datas = [seed + seed[:L] + bytes([(seed[L] + 1) & 63]) for L in range(3, 259)]
    got = round_trip(datas, (1, 9), "every length")
    seen = set()
    for walks in got[(9, 0)][1]:
        for b in walks:
            for t in b["tokens"]:
                if t[0] == "match":
                    seen.add(t[3])
                    assert (t[3] == 285) == (t[1] == 258), "length 258 is symbol 285 with no extra bits"
    assert seen == set(range(257, 286)), sorted(set(range(257, 286)) - seen)


def test_every_distance_code():
    base = rnd(32832, 6)
    ds = sorted(set(list(range(1, 9)) + [R for d in range(4, 30) for R in (W.R.DIST_BASE[d], W.R.DIST_BASE[d] + (1 << W.R.DIST_EXTRA[d]) - 1)]))
    assert ds[-1] == 32768 and 24577 in ds and 16385 in ds and 24576 in ds
    buf, fresh = bytearray(base), random.Random(7)
    for d in ds:
        for _ in range(8):
            buf.append(buf[-d])
        buf.append(fresh.randrange(256))
    round_trip([bytes(buf)], (1, 6, 9), "every distance code")


def test_too_far():
    a, b, c = rnd(40000, 8), rnd(32768, 9), rnd(32769, 10)
    datas = [a + a[:1000], b + b, c + c]
    got = round_trip(datas, (1, 9), "too far")
    for level in (1, 9):
        walks = got[(level, 0)][1]
        far = [t for blk in walks[0] for t in blk["tokens"] if t[0] == "match" and t[1] > 5]
        assert not far, "the only source lies 40 000 back: %r" % far[:3]
        assert not [t for blk in walks[2] for t in blk["tokens"] if t[0] == "match" and t[1] > 5]


def test_block_edges(test_bmp):
    b = B()
    datas = [test_bmp[:n] for n in (b - 1, b, b + 1, 2 * b, 2 * b + 1, 3 * b + 7)]
    x = bytearray(rnd(2 * b, 11))
    x[b - 300:b + 300] = b"\x55" * 600
    y = bytearray(rnd(2 * b, 12))
    y[b:b + 300] = y[b - 300:b]
    datas += [bytes(x), bytes(y)]
    got = round_trip(datas, (1, 6), "block edges")
    for level in (1, 6):
        outs, walks = got[(level, 0)]
        # the run and the copy are found on both sides of the edge: the history of a block is the input in front of it
        for k in (6, 7):
            long_ones = [(blk["start"], t) for blk in walks[k] for t in blk["tokens"] if t[0] == "match" and t[1] >= 100]
            assert any(s >= b for s, _ in long_ones), (level, k, long_ones)


def test_stored(test_bmp):
    datas = [rnd(n, n) for n in (65535, 65536, 65537)]
    for level in (0, 6):
        got = round_trip(datas, (level,), "stored")
        for flags in (0, A.DEFLATE_FIXED):
            for d, o, walks in zip(datas, *got[(level, flags)]):
                assert len(o) <= bound(len(d))
                assert level or all(blk["type"] == W.STORED for blk in walks), "level 0 writes stored blocks only"
    got = round_trip([test_bmp[:3 * B() + 5]], (0,), "stored bmp")
    assert all(blk["type"] == W.STORED for blk in got[(0, 0)][1][0])


def test_flat_and_skewed():
    perm = list(range(256))
    random.Random(13).shuffle(perm)
    r = random.Random(14)
    datas = [bytes(perm) * 16, bytes(r.choice(b"xyz") for _ in range(4096))]
    got = round_trip(datas, (1, 6, 9), "flat and skewed")
    assert len(got[(6, 0)][0][1]) < 4096 * 2 // 8 + 120, "three values take under two bits each"


def test_capacity():
    datas = [IC.text_like(5000, 1), rnd(700, 2), IC.text_like(B() + 900, 3), b"", b"q" * 999]
    for level, flags in ((0, 0), (6, 0), (6, A.DEFLATE_FIXED)):
        res, outs = encode(datas, level, flags, what="capacity: bound")
        assert all(st == A.ST_OK for st, _ in res)
        res2, outs2 = encode(datas, level, flags, caps=[len(o) for o in outs], what="capacity: exact")
        assert (res2, outs2) == (res, outs)
        caps = [len(o) - (1 if i in (0, 2, 3) else 0) for i, o in enumerate(outs)]
        res3, outs3 = encode(datas, level, flags, caps=caps, what="capacity: one short")
        for i in range(len(datas)):
            if i in (0, 2, 3):
                assert res3[i] == (A.ST_OUTPUT_CAPACITY, 0), i
            else:
                assert (res3[i], outs3[i]) == (res[i], outs[i]), i


def test_independence():
    r = random.Random(15)
    small = [IC.text_like(r.randrange(1, 201), k) if k % 2 else rnd(r.randrange(1, 201), k) for k in range(3000)]
    big = IC.text_like(5 * B() + 123, 16)
    c = ctx()
    for level in (1, 6):
        items = [dict(src=d, cap=bound(len(d))) for d in small[:1500] + [big] + small[1500:]]
        streams, src, dst_bytes = TG.pack(items)
        dst, res = c.deflate_encode_batch(streams, src, dst_bytes, level, 0)
        outs = [dst[streams[i].dst_off:streams[i].dst_off + res[i].dst_len].tobytes() for i in range(len(items))]
        assert all(res[i].status == A.ST_OK for i in range(len(items)))
        (_, alone), = [encode([big], level, 0, what="independence: alone")]
        assert outs[1500] == alone[0], "the batch around a stream changes its bytes"
        datas = [it["src"] for it in items]
        read_back(datas, outs, level, 0, "independence", walk=False)
        for i in range(0, len(items), 97):
            walk_check(datas[i], outs[i], level, 0, "independence stream %d" % i)
        walk_check(big, alone[0], level, 0, "independence: the long stream")


def test_refusals_and_the_empty_batch():
    c = ctx()
    L = lib()
    st = (A.Stream * 1)(A.Stream(0, 0, 4, 64, 0, 0, 0, 0))
    res = (A.Result * 1)()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    assert L.alz_deflate_encode_batch(c.h, 6, 0, 0, None, 0, None, None, 0, None) == 0
    assert L.alz_deflate_file_compress_batch(c.h, 6, 0, 0, None, 0, None, None, 0, None) == 0
    for level, flags in ((-1, 0), (10, 0), (6, 2), (6, 3)):
        assert L.alz_deflate_encode_batch(c.h, level, flags, 1, src, 64, st, dst, 64, res) == A.E_INVALID
        assert L.alz_deflate_file_compress(c.h, A.ZFILE_ZLIB, level, flags, src, 4, dst, 64, None) == A.E_INVALID
    assert L.alz_deflate_file_compress(c.h, 2, 6, 0, src, 4, dst, 64, None) == A.E_INVALID


# ---------------------------------------------------------------------------------------------- files
def file_compress(kind, level, flags, data, cap=None):
    L = lib()
    cap = L.alz_deflate_file_bound(kind, len(data)) if cap is None else cap
    dst = np.full(cap + 16, GUARD, dtype=np.uint8)
    dl = C.c_size_t(12345)
    rc = L.alz_deflate_file_compress(ctx().h, kind, level, flags, bytes(data), len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl))
    assert (dst[cap:] == GUARD).all()
    return rc, dst[:dl.value].tobytes()


def test_files_single(test_bmp):
    L = lib()
    zhead = {0: b"\x78\x01", 1: b"\x78\x01", 6: b"\x78\x9c", 9: b"\x78\xda"}
    xfl = {0: 4, 1: 4, 6: 0, 9: 2}
    datas = [b"", b"abc", IC.text_like(3000, 2), test_bmp[:B() + 77]]
    for level in LEVELS:
        for d in datas:
            rc, z = file_compress(A.ZFILE_ZLIB, level, 0, d)
            assert rc == 0 and z[:2] == zhead[level] and zlib.decompress(z) == d and z[-4:] == zlib.adler32(d).to_bytes(4, "big")
            rc, g = file_compress(A.ZFILE_GZIP, level, 0, d)
            assert rc == 0 and g[:10] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00" + bytes([xfl[level], 3]) and gzip.decompress(g) == d
            assert g[-8:] == zlib.crc32(d).to_bytes(4, "little") + len(d).to_bytes(4, "little")
            for fn, f in (("alz_zlib_decompress", z), ("alz_gzip_decompress", g)):
                out = np.zeros(len(d) + 8, dtype=np.uint8)
                dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
                assert getattr(L, fn)(ctx().h, f, len(f), out.ctypes.data_as(C.c_void_p), len(d) + 8, C.byref(dl), C.byref(su), C.byref(st)) == 0
                assert (dl.value, su.value) == (len(d), len(f)) and out[:len(d)].tobytes() == d
            if len(d) >= 3:
                assert L.alz_zlib_is_match(z, len(z)) == 1 and L.alz_gzip_is_match(g, len(g)) == 1
            # a capacity one byte short is ALZ_E_NOMEM, the exact one is enough
            assert file_compress(A.ZFILE_ZLIB, level, 0, d, cap=len(z))[1] == z and file_compress(A.ZFILE_ZLIB, level, 0, d, cap=len(z) - 1)[0] == A.E_NOMEM
            assert file_compress(A.ZFILE_GZIP, level, 0, d, cap=len(g) - 1)[0] == A.E_NOMEM
    assert file_compress(A.ZFILE_GZIP, 6, 0, b"abc", cap=17)[0] == A.E_NOMEM and file_compress(A.ZFILE_ZLIB, 6, 0, b"abc", cap=5)[0] == A.E_NOMEM


def test_files_batch_equals_the_single_file_call(test_bmp):
    L = lib()
    r = random.Random(17)
    b = B()
    datas = []
    for k in range(40):
        n = (0, 1, b, 3 * b)[k] if k < 4 else r.randrange(0, 3 * b) if k % 5 == 0 else r.randrange(0, 4000)
        o = r.randrange(0, len(test_bmp) - n)
        datas.append(test_bmp[o:o + n] if k % 3 else rnd(n, k))
    for level, flags in ((6, 0), (1, A.DEFLATE_FIXED)):
        kinds = [k % 2 for k in range(40)]
        singles = [file_compress(kinds[k], level, flags, datas[k]) for k in range(40)]
        caps = [L.alz_deflate_file_bound(kinds[k], len(datas[k])) for k in range(40)]
        for k in (7, 22):
            caps[k] = len(singles[k][1]) - 1
            singles[k] = file_compress(kinds[k], level, flags, datas[k], cap=caps[k])
            assert singles[k][0] == A.E_NOMEM
        items = [dict(src=datas[k], cap=caps[k]) for k in range(40)]
        files, src, dst_bytes = TG.pack(items)
        for k in range(40):
            files[k].format = kinds[k]
        dst, res = ctx().deflate_file_compress_batch(files, src, dst_bytes, level, flags, dst=np.full(dst_bytes, GUARD, dtype=np.uint8))
        mask = np.ones(dst.size, dtype=bool)
        for k in range(40):
            rc, f = singles[k]
            a = files[k].dst_off
            assert (res[k].rc, res[k].status, res[k].dst_len, res[k].src_used) == (rc, A.ST_OK, len(f), len(datas[k]) if rc == 0 else 0), (level, k)
            assert dst[a:a + len(f)].tobytes() == f, (level, k)
            mask[a:a + len(f)] = False
        assert (dst[mask] == GUARD).all()
    files[3].format = 2
    with pytest.raises(_lib.AlzError):
        ctx().deflate_file_compress_batch(files, src, dst_bytes, 6, 0)


def test_python_classes(test_bmp):
    xs = [b"", b"hello hello hello", IC.text_like(70000, 3), test_bmp[1000:9000]]
    for cls in (F.ZLib, F.GZip):
        many = cls().DeflateMany(xs, level=6)
        assert many == [cls().Deflate(x, level=6) for x in xs]
        assert cls().DecompressMany(many) == xs
        assert cls().Deflate(xs[2], level=1, fixed=True) == cls().DeflateMany([xs[2]], level=1, fixed=True)[0]
        assert cls().Decompress(cls().Deflate(xs[3], *cls().DeflateLevel(F.CompressionSettings.Maximum))) == xs[3]
    assert zlib.decompress(F.ZLib().Deflate(xs[2], 9)) == xs[2] and gzip.decompress(F.GZip().Deflate(xs[2], 0)) == xs[2]


# ---------------------------------------------------------------------------------------------- ratio
def test_ratio_against_zlib(test_bmp):
    wins = [test_bmp[k * 65536:(k + 1) * 65536] for k in range(16)]
    total = sum(len(w) for w in wins)

    def ztotal(level, strategy=zlib.Z_DEFAULT_STRATEGY):
        return sum(len(IC.raw_deflate(w, level, strategy)) for w in wins)

    z1, huff = ztotal(1), ztotal(6, zlib.Z_HUFFMAN_ONLY)
    items = [dict(src=w, cap=bound(len(w))) for w in wins]
    streams, src, dst_bytes = TG.pack(items)
    ours = {}
    for level in range(1, 10):
        dst, res = ctx().deflate_encode_batch(streams, src, dst_bytes, level, 0)
        assert all(res[i].status == A.ST_OK for i in range(16))
        ours[level] = sum(res[i].dst_len for i in range(16))
        if level in (1, 9):
            read_back(wins, [dst[streams[i].dst_off:streams[i].dst_off + res[i].dst_len].tobytes() for i in range(16)], level, 0, "ratio", walk=False)
    print("zlib level 1 %.4f, Z_HUFFMAN_ONLY %.4f; GPU levels 1..9: %s" % (z1 / total, huff / total, " ".join("%.4f" % (ours[l] / total) for l in range(1, 10))))
    for level in range(1, 10):
        assert ours[level] < huff, "level %d: %d bytes, zlib's Z_HUFFMAN_ONLY %d: the finder finds nothing" % (level, ours[level], huff)
    assert ours[9] <= 1.10 * z1, "level 9: %d bytes, zlib level 1: %d" % (ours[9], z1)
