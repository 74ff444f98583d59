"""-m gpu: the wrapped-file layer (alz_wfile_*) on the device, under the exact and the production context modes.  Every file of the CPU corpus
(tests/wfile_ref.py) through alz_wfile_decompress against the standard library's bytes and the expected rc / status; the whole corpus as one mixed
alz_wfile_decode_batch and as batches of one against the single-file results, field for field and byte for byte; a 40-chunk HWGZ file, a
3-chunk ZLWF file; every kind written by alz_wfile_compress and read back, RLHudson and ZLWF bit-identical to the managed bytes."""
import ctypes as C
import struct

import numpy as np
import pytest

import rlhudson_ref as RH
import wfile_ref as W
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from gpu_common import ctx

pytestmark = pytest.mark.gpu
FAMILIES = ((1, "exact"), (0, "production"))


def single(kind, big, f, cap):
    """alz_wfile_decompress -> (rc, status, dst_len, src_used, bytes)"""
    o = A.ContainerOptions()
    o.big_endian = big
    dst = np.full(cap + 16, 0xA5, dtype=np.uint8)
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = ctx().lib.alz_wfile_decompress(ctx().h, kind, C.byref(o), f, len(f), dst.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
    assert (dst[cap:] == 0xA5).all()
    return rc, st.value, dl.value, su.value, dst[:dl.value].tobytes()


def cap_of(c):
    return c[4]["stated"] + 64 if c[4] else len(c[5]) + 64


def both_families(fn):
    for exact, fam in FAMILIES:
        ctx().set_exact_kernels(exact)
        try:
            fn(fam)
        finally:
            ctx().set_exact_kernels(0)


def test_corpus_single_files():
    def run(fam):
        for c in W.corpus():
            name, kind, big, f, want, data, expect = c
            rc, st, dl, su, out = single(kind, big, f, cap_of(c))
            tag = "%s [%s]" % (name, fam)
            print("%s: rc=%d status=%d dst_len=%d src_used=%d" % (tag, rc, st, dl, su))
            if expect is None:                                        # the body's reference decides
                ref = RH.rlhudson_decode(f[8:], want["stated"], cap_of(c))
                assert (st, dl, out) == (ref[1], ref[2], ref[0]) and rc == (0 if ref[1] == 0 else A.E_STREAM), tag
                continue
            assert (rc, st) == expect, tag
            if rc in (0, A.E_CHECKSUM) or st == A.ST_OUTPUT_SIZE_MISMATCH:
                assert out == data and dl == len(data), tag           # the output is delivered
            else:
                assert data is None or out == data[:dl], tag
            if rc == 0:
                assert 0 < su <= len(f), tag
            if st == A.ST_INPUT_TRUNCATED and kind not in (W.ASURAZLB, W.ZLB, W.HWGZ):
                assert su == len(f), tag
    both_families(run)


def test_keystream_700_words():
    """an encrypted, uncompressed SSZL file whose stored bytes are zeros decodes to the library's keystream: 700 words of it (they cross the 624-word
    state) and the tails of 1-3 bytes, which take one more word, against the restatement of tests/wfile_ref.py"""
    want = b"".join(struct.pack("<I", w) for w in W.sszl_keystream(701))
    for tail in (0, 1, 2, 3):
        n = 2800 + tail
        f = b"SSZL" + struct.pack("<IIII", 0x20101109, n, W.ENCRYPTED, 0) + bytes(n)
        assert single(W.SSZL, 0, f, n + 64) == (0, 0, n, len(f), want[:n]), tail


def batch(cases, caps=None):
    n = len(cases)
    files = (A.Stream * n)()
    so, do, chunks = 0, 0, []
    for i, c in enumerate(cases):
        cap = caps[i] if caps else cap_of(c)
        do = (do + 48 + 15) // 16 * 16 + (i % 4) * 5
        files[i] = A.Stream(so, do, len(c[3]), cap, 0, c[2], 0, c[1])
        chunks.append(c[3])
        so += len(c[3]); do += cap
    dst = np.full(do + 64, 0xA5, dtype=np.uint8)
    dst, res = ctx().wfile_decode_batch(files, np.frombuffer(b"".join(chunks) + bytes(1), dtype=np.uint8), do + 64, dst=dst)
    touched = np.zeros(do + 64, dtype=bool)
    for i in range(n):
        touched[files[i].dst_off:files[i].dst_off + res[i].dst_len] = True
    assert not np.any(~touched & (dst != 0xA5)), "a byte outside the files' outputs changed"
    return [(res[i].rc, res[i].status, res[i].dst_len, res[i].src_used, dst[files[i].dst_off:files[i].dst_off + res[i].dst_len].tobytes()) for i in range(n)]


def test_mixed_batch_is_the_single_file_results():
    cases = W.corpus()
    # ... and prefixes of one file per kind: whatever each ends in, the batch says what the single call says
    seen = set()
    for c in list(cases):
        if c[4] is not None and c[1] not in seen:
            seen.add(c[1])
            for cut in (0, 3, 7, 11, 19, len(c[3]) // 2, len(c[3]) - 5, len(c[3]) - 1):
                cases.append((c[0] + ", first %d bytes" % cut, c[1], c[2], c[3][:cut], c[4], c[5], None))

    def run(fam):
        want = [single(c[1], c[2], c[3], cap_of(c)) for c in cases]
        for i, (c, w) in enumerate(zip(cases, want)):
            if "first" in c[0]:
                assert w[0] in (0, A.E_FORMAT, A.E_STREAM, A.E_CHECKSUM), c[0]
                if w[0] == 0:
                    assert w[4] == c[5], c[0]                          # (a bounded body that lost only trailer bytes)
        got = batch(cases)
        for c, w, g in zip(cases, want, got):
            assert g == w, "%s [%s]: batch %r, single %r" % (c[0], fam, g[:4], w[:4])
        for c, w in zip(cases, want):                                 # batches of one, every case
            assert batch([c]) == [w], "%s [%s], alone" % (c[0], fam)
        # a capacity one below the need: OUTPUT_CAPACITY, and the same in both
        tight = [c for c in cases if c[6] == (0, 0)][:16]
        caps = [len(c[5]) - 1 for c in tight]
        tw = [single(c[1], c[2], c[3], cap) for c, cap in zip(tight, caps)]
        assert all(w[:2] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY) for w in tw), [w[:3] for w in tw]
        assert batch(tight, caps) == tw
    both_families(run)


def test_hwgz_of_40_chunks_and_zlwf_of_3():
    d = W.sample(40 * 4096 - 100, 77)
    hw, hf = W.hwgz(d, 4096, header_big=False, order_big=True)
    zl, zf = W.zlwf(d[:3 * 5000 - 7], 5000, big=False)
    assert len(hf["parts"]) == 40 and len(zf["parts"]) == 3

    def run(fam):
        assert single(W.HWGZ, 1, hw, len(d) + 64)[:3] + (single(W.HWGZ, 1, hw, len(d) + 64)[4],) == (0, 0, len(d), d)
        assert single(W.ZLWF, 0, zl, 15000)[:3] + (single(W.ZLWF, 0, zl, 15000)[4],) == (0, 0, 3 * 5000 - 7, d[:3 * 5000 - 7])
        h, z = F.HWGZ(), F.ZLWF()
        z.FormatByteOrder = "Little"
        assert h.Decompress(hw) == d and z.Decompress(zl) == d[:3 * 5000 - 7] and h.DecompressMany([hw, hw[:300], hw])[0] == d
        assert isinstance(h.DecompressMany([hw, hw[:300]])[1], F.EndOfStreamException)
        # a chunk with a flipped Adler-32 in the middle: the file ends there with its output delivered
        bad = bytearray(hw)
        off, ln = hf["parts"][20][0], hf["parts"][20][1]
        bad[off + ln - 1] ^= 1
        rc, st, dl, su, out = single(W.HWGZ, 1, bytes(bad), len(d) + 64)
        assert (rc, dl, out) == (A.E_CHECKSUM, 21 * 4096, d[:21 * 4096])
    both_families(run)


def test_writers_read_back():
    d = W.sample(70000, 5)
    small = W.sample(900, 6)

    def run(fam):
        for cls in F.WRAPPED_FORMATS:
            for data in (d, small, b"x"):
                obj = cls()
                if cls is F.HWGZ:
                    obj.ChunkSize = 0x4000
                if cls is F.ZLWF:
                    obj.BlockSize = 0x8000
                for order in (("Big", "Little") if cls in (F.HWGZ, F.ZLWF) else ("Big",)):
                    obj.FormatByteOrder = order
                    for opts in ((0, 1, 0x80000000, 0x80000001, 0x80000003) if cls is F.SSZL else (None,)):
                        if opts is not None:
                            obj.Options = opts
                        if opts == 0:
                            continue                                   # (0 asks the writer for the class default)
                        f = obj.Deflate(data) if cls.deflate else obj.Compress(data)
                        tag = "%s %s %s %d bytes [%s]" % (cls.__name__, order, opts, len(data), fam)
                        assert obj.IsMatch(f) or len(f) <= 0x14 or (cls is F.HWGZ and len(f) < 0x80), tag
                        assert obj.GetDecompressedSize(f) == len(data), tag
                        # (ZLB's stated compressed size is four short, as the reference writes it: the reader stops in front of the Adler-32)
                        assert obj.Decompress(f) == data and obj.last_src_used == len(f) - (4 if cls is F.ZLB else 0), tag
                        if cls.deflate:
                            with pytest.raises(NotImplementedError):
                                obj.Compress(data)
        # the managed bytes: RLHudson's header + the restated body; ZLWF's header, table and alignment around the WFLZ files of the container layer
        assert F.RLHudson().Compress(small) == W.rlhudson(small)[0]
        z, w = F.ZLWF(), F.WFLZ()
        z.BlockSize, w.FormatByteOrder = 400, "Big"
        want = bytearray(b"ZLWF" + bytes(4) + struct.pack(">II", len(small), 3) + bytes(12))
        for i in range(3):
            want += bytes(-len(want) % 16)
            struct.pack_into(">I", want, 16 + 4 * i, len(want))
            want += w.Compress(small[400 * i:400 * i + 400])
        want += bytes(-len(want) % 16)
        struct.pack_into(">I", want, 4, len(want) - 16)
        assert z.Compress(small) == bytes(want)
        # the header fields of the DEFLATE kinds, as the reference's header code writes them
        f = F.ZLB().Deflate(small)
        assert f[:4] == b"ZLB\0" and struct.unpack(">III", f[4:16]) == (1, len(small), len(f) - 0x14)
        f = F.AsuraZlb().Deflate(small)
        assert f[:12] == b"AsuraZlb\1\0\0\0" and struct.unpack(">II", f[12:20]) == (len(f) - 0x14, len(small))
        h = F.HWGZ()
        h.ChunkSize = 256
        f = h.Deflate(small)
        parts = h.Walk(f)[0]
        assert struct.unpack(">III", f[:12]) == (256, 4, len(small)) and list(struct.unpack(">4I", f[12:28])) == [p[1] + 4 for p in parts]
        s = F.SSZL()
        s.Options = 0x80000003
        f = s.Deflate(small)
        assert struct.unpack("<IIII", f[4:20]) == (0x20101109, len(small), 0x80000001, 0) and W.sszl_xor(f[20:])[:2] == b"\x1f\x8b"
        assert s.Decompress(f) == small and s.Options == 0x80000001
    both_families(run)
