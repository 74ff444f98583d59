"""-m gpu: ZLib and GZip files in batches (alz_zfile_decode_batch, alz_zfile_measure_batch, DecompressMany).  The contract is differential:
for every file the batch returns the (rc, status, dst_len, src_used) and delivers the bytes of the single-file call (alz_zlib_decompress /
alz_gzip_decompress / their measure twins) on the same context with the same capacity; valid files are held against the standard library's
zlib / gzip as well.  Every destination lies between guard bytes.  Every comparison is exact."""
import ctypes as C
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

import test_inflate_cpu as IC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 0xA5
Z, G = A.ZFILE_ZLIB, A.ZFILE_GZIP
FN = {Z: "alz_zlib", G: "alz_gzip"}


def gz(payload, flags=0, level=6, crc=None, isize=None):
    """one gzip member, written by hand so that every optional header field can be set"""
    h = b"\x1f\x8b\x08" + bytes([flags]) + bytes(4) + b"\x00\xff"
    if flags & 4:
        h += struct.pack("<H", 7) + b"extra!!"
    if flags & 8:
        h += b"file.bin\0"
    if flags & 16:
        h += b"a comment\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + IC.raw_deflate(payload, level) + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize)


def flip_stored_payload(f, plain):
    """a level-0 file with one payload byte flipped: the body still decodes, only the checksum can tell"""
    at = f.index(plain[:32]) + len(plain) // 2
    return f[:at] + bytes([f[at] ^ 0x40]) + f[at + 1:], plain[:len(plain) // 2] + bytes([plain[len(plain) // 2] ^ 0x40]) + plain[len(plain) // 2 + 1:]


_CORPUS = None


def corpus():
    """[dict(fmt, data, cap, name, plain)]: cap None = the true size; plain: the bytes of a valid file, std: the standard library reads it too"""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    rng = random.Random(1952)
    text, noise = IC.text_like(3000, 7), rng.randbytes(1500)
    out = []

    def add(fmt, data, name, cap=None, plain=None, std=True):
        out.append(dict(fmt=fmt, data=bytes(data), cap=cap, name=name, plain=plain, std=std and plain is not None))
    for level in (0, 1, 6, 9):
        add(Z, zlib.compress(text, level), "zlib level %d" % level, plain=text)
    add(Z, zlib.compress(noise, 6), "zlib noise", plain=noise)
    add(Z, zlib.compress(b"", 6), "zlib of nothing", plain=b"")
    add(G, gz(text), "gzip plain", plain=text)
    add(G, gzip.compress(noise, mtime=0), "gzip of the standard library", plain=noise)
    for flags, nm in ((4, "FEXTRA"), (8, "FNAME"), (16, "FCOMMENT"), (2, "FHCRC"), (30, "all four")):
        add(G, gz(text, flags), "gzip " + nm, plain=text)
    add(G, gz(text) + gz(noise, 8), "gzip two members", plain=text + noise)
    add(G, gz(text, 2) + gz(b"") + gz(noise, 0, 1), "gzip three members", plain=text + noise)
    add(G, gz(text) + b"garbage behind the member", "gzip trailing garbage", plain=text, std=False)
    add(G, gz(text) + b"\x1f", "gzip one trailing byte", plain=text, std=False)
    for fmt in (Z, G):
        add(fmt, b"", "empty file %d" % fmt)
        add(fmt, b"\x78" if fmt == Z else b"\x1f", "one-byte file %d" % fmt)
    z, g = zlib.compress(text, 6), gz(text, 30)
    add(Z, b"\x79\x9c" + z[2:], "zlib CM 9")
    add(Z, b"\x78\x9d" + z[2:], "zlib bad FCHECK")
    add(Z, b"\x78\xbb" + z[2:], "zlib FDICT")
    add(G, b"\x1f\x8c" + g[2:], "gzip bad magic")
    add(G, g[:3] + b"\x40" + g[4:], "gzip reserved flag")
    add(G, g[:20] + bytes([g[20] ^ 1]) + g[21:], "gzip FHCRC mismatch")
    for cut in (1, 5, 9, 14, 25):
        add(G, g[:cut], "gzip cut in the header at %d" % cut)
    add(Z, z[:1], "zlib cut in the header")
    add(Z, z[:2], "zlib header only")
    add(Z, z[:len(z) // 2], "zlib cut in the body")
    add(G, g[:len(g) - 200], "gzip cut in the body")
    for k in range(1, 5):
        add(Z, z[:-k], "zlib trailer cut by %d" % k)
    for k in range(1, 9):
        add(G, g[:-k], "gzip trailer cut by %d" % k)
    for fmt, f in ((Z, z), (G, g)):
        add(fmt, f, "capacity 0 (%d)" % fmt, cap=0)
        add(fmt, f, "capacity one short (%d)" % fmt, cap=len(text) - 1)
        add(fmt, f, "capacity exact (%d)" % fmt, cap=len(text), plain=text)
        add(fmt, f, "capacity generous (%d)" % fmt, cap=len(text) + 100, plain=text)
    add(Z, z[:-1] + bytes([z[-1] ^ 1]), "zlib wrong Adler-32")
    add(G, gz(text, crc=zlib.crc32(text) ^ 0x100), "gzip wrong CRC-32")
    add(G, gz(text, isize=len(text) + 1), "gzip wrong ISIZE")
    two = gz(text) + gz(noise)
    add(G, two[:-3], "gzip second member: trailer cut")
    add(G, gz(text) + gz(noise, crc=5), "gzip second member: wrong CRC-32")
    add(G, gz(text) + gz(noise)[:40], "gzip second member: body cut")
    add(G, gz(text) + b"\x1f\x8b\x09" + bytes(20), "gzip second member: bad header")
    add(G, two, "gzip second member does not fit", cap=len(text) + 10)
    add(G, two, "gzip first member fills the capacity", cap=len(text))
    for fmt, f in ((Z, zlib.compress(text, 0)), (G, gz(text, level=0))):
        bad, flipped = flip_stored_payload(f, text)
        add(fmt, bad, "stored block with a flipped payload byte (%d)" % fmt)
        out[-1]["flipped"] = flipped
    _CORPUS = out
    return out


def cap_of(it):
    if it["cap"] is not None:
        return it["cap"]
    return len(it["plain"]) if it["plain"] is not None else 4096


_SINGLE = {}


def single(k, measure=False, limit=None):
    """the single-file call on corpus item k, once: ((rc, status, dst_len, src_used), the bytes delivered)"""
    key = (k, measure, limit)
    if key in _SINGLE:
        return _SINGLE[key]
    it, c = corpus()[k], ctx()
    data = it["data"]
    dl, su, st = C.c_size_t(777), C.c_size_t(777), C.c_int32(77)
    if measure:
        rc = getattr(c.lib, FN[it["fmt"]] + "_measure")(c.h, data, len(data), cap_of(it) if limit is None else limit, C.byref(dl), C.byref(su), C.byref(st))
        got = b""
    else:
        cap = cap_of(it)
        dst = np.full(cap + 1, GUARD, dtype=np.uint8)
        rc = getattr(c.lib, FN[it["fmt"]] + "_decompress")(c.h, data, len(data), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
        assert dl.value <= cap and dst[cap] == GUARD
        got = dst[:dl.value].tobytes()
    _SINGLE[key] = ((rc, st.value, dl.value, su.value), got)
    return _SINGLE[key]


def pack(ks, limit=None):
    """(files, src, dst_bytes, dst offsets): file j is corpus item ks[j]; sources at every residue mod 16, destinations between guard gaps"""
    items = corpus()
    files = (A.Stream * len(ks))()
    chunks, so, do = [], 0, 16
    for j, k in enumerate(ks):
        it, mis = items[k], j % 16
        chunks.append(bytes([0xEE]) * mis + it["data"])
        do += 1 + (j * 7) % 23
        files[j] = A.Stream(so + mis, do, len(it["data"]), cap_of(it) if limit is None else limit, 0xDEAD, 0xBEEF, 0xF00D, it["fmt"])
        so += len(chunks[-1])
        do += cap_of(it)
    return files, np.frombuffer(b"".join(chunks) + bytes(1), dtype=np.uint8), do + 16


def check_decode(ks):
    items = corpus()
    files, src, dst_bytes = pack(ks)
    dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
    out, res = ctx().zfile_decode_batch(files, src, dst_bytes, dst=dst)
    assert out is dst
    covered = np.zeros(dst_bytes, dtype=bool)
    for j, k in enumerate(ks):
        it, r = items[k], res[j]
        want, want_bytes = single(k)
        a = int(files[j].dst_off)
        assert (r.rc, r.status, r.dst_len, r.src_used) == want, (it["name"], j, (r.rc, r.status, r.dst_len, r.src_used), want)
        assert dst[a:a + r.dst_len].tobytes() == want_bytes, (it["name"], j)
        if it["plain"] is not None:
            assert (r.rc, r.dst_len) == (0, len(it["plain"])) and want_bytes == it["plain"], (it["name"], j)
        covered[a:a + int(files[j].dst_cap)] = True
    assert (dst[~covered] == GUARD).all(), "bytes between two destinations were written"


def test_the_corpus_is_what_it_claims():
    seen = set()
    for k, it in enumerate(corpus()):
        if it["std"]:
            assert (zlib.decompress(it["data"]) if it["fmt"] == Z else gzip.decompress(it["data"])) == it["plain"], it["name"]
        seen.add(single(k)[0][:2])
    for need in ((0, A.ST_OK), (A.E_FORMAT, A.ST_OK), (A.E_UNSUPPORTED, A.ST_OK), (A.E_CHECKSUM, A.ST_OK), (A.E_STREAM, A.ST_INPUT_TRUNCATED), (A.E_STREAM, A.ST_OUTPUT_CAPACITY)):
        assert need in seen, (need, seen)


def test_every_file_of_the_corpus_in_one_batch():
    check_decode(list(range(len(corpus()))))


def test_batches_of_one_file():
    for k in (0, 6, 13, len(corpus()) - 1):
        check_decode([k])


def test_the_checksum_is_in_the_loop():
    items = corpus()
    ks = [k for k, it in enumerate(items) if "flipped" in it]
    assert sorted(items[k]["fmt"] for k in ks) == [Z, G]
    files, src, dst_bytes = pack(ks)
    dst, res = ctx().zfile_decode_batch(files, src, dst_bytes)
    for j, k in enumerate(ks):
        a, want = int(files[j].dst_off), items[k]["flipped"]
        assert (res[j].rc, res[j].status, res[j].dst_len) == (A.E_CHECKSUM, A.ST_OK, len(want)), (items[k]["name"], res[j].rc)
        assert dst[a:a + len(want)].tobytes() == want
        assert single(k)[0][0] == A.E_CHECKSUM


def test_a_mixed_batch_of_1500_files():
    rng = random.Random(1500)
    n = len(corpus())
    ks = [rng.randrange(n) for _ in range(1500)]
    rng.shuffle(ks)
    assert {corpus()[k]["fmt"] for k in ks} == {Z, G}
    check_decode(ks)


def test_measure_equals_the_single_file_measure():
    items = corpus()
    ks = list(range(len(items)))
    files, src, _ = pack(ks)
    res = ctx().zfile_measure_batch(files, src)
    for j, k in enumerate(ks):
        want = single(k, measure=True)[0]
        assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == want, (items[k]["name"], want)
    # the size itself, and a limit below it
    good = [k for k, it in enumerate(items) if it["plain"] and it["cap"] is None]
    assert len(good) >= 12
    files, src, _ = pack(good, limit=A.MEASURE_NO_BOUND)
    res = ctx().zfile_measure_batch(files, src)
    for j, k in enumerate(good):
        assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == single(k, True, A.MEASURE_NO_BOUND)[0]
        assert (res[j].rc, res[j].dst_len) == (0, len(items[k]["plain"])), items[k]["name"]
    files, src, _ = pack(good, limit=100)
    res = ctx().zfile_measure_batch(files, src)
    for j, k in enumerate(good):
        assert (res[j].rc, res[j].status, res[j].dst_len) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, 100), items[k]["name"]
        assert (res[j].rc, res[j].status, res[j].dst_len, res[j].src_used) == single(k, True, 100)[0]


def test_arguments():
    c = ctx()
    it = corpus()[0]
    files, src, dst_bytes = pack([0])
    dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
    res = (A.FileResult * 1)()
    sp, dp = src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p)
    assert c.lib.alz_zfile_decode_batch(c.h, 0, None, 0, None, None, 0, None) == 0 and c.lib.alz_zfile_measure_batch(c.h, 0, None, 0, None, None) == 0
    files[0].format = 2
    assert c.lib.alz_zfile_decode_batch(c.h, 1, sp, src.nbytes, files, dp, dst_bytes, res) == A.E_INVALID    # an unknown format
    assert c.lib.alz_zfile_measure_batch(c.h, 1, sp, src.nbytes, files, res) == A.E_INVALID
    files[0].format = it["fmt"]
    assert c.lib.alz_zfile_decode_batch(c.h, 1, sp, len(it["data"]) - 1, files, dp, dst_bytes, res) == A.E_INVALID     # the file outside src_bytes
    assert c.lib.alz_zfile_decode_batch(c.h, 1, sp, src.nbytes, files, dp, int(files[0].dst_off), res) == A.E_INVALID   # the destination outside dst_bytes
    assert c.lib.alz_zfile_decode_batch(c.h, 1, sp, src.nbytes, None, dp, dst_bytes, res) == A.E_INVALID
    assert c.lib.alz_zfile_decode_batch(c.h, 1, sp, src.nbytes, files, dp, dst_bytes, None) == A.E_INVALID
    assert (dst == GUARD).all()


@pytest.mark.parametrize("cls,fmt", ((F.ZLib, Z), (F.GZip, G)), ids=("ZLib", "GZip"))
def test_decompress_many(cls, fmt):
    items = [it for it in corpus() if it["fmt"] == fmt and it["cap"] is None]
    assert sum(it["plain"] is not None for it in items) >= 6 and sum(it["plain"] is None for it in items) >= 10
    f = cls()
    got = f.DecompressMany([it["data"] for it in items])
    assert len(got) == len(items) and f.DecompressMany([]) == []
    kinds = set()
    for it, g in zip(items, got):
        try:
            want = f.Decompress(it["data"])
        except Exception as e:
            want = e
        if isinstance(want, bytes):
            assert g == want and (it["plain"] is None or g == it["plain"]), it["name"]
        else:
            assert it["plain"] is None and type(g) is type(want), (it["name"], g, want)
            kinds.add(type(want))
    assert {F.InvalidIdentifierException, F.InvalidDataException, F.EndOfStreamException} <= kinds, kinds
