"""No GPU: DEFLATE (alz_inflate_*, alz_zlib_*, alz_gzip_*).  The pure-Python reference decoder and assembler (tests/inflate_ref.py) against the
standard library's zlib -- valid streams of every level and strategy, every byte-prefix, single-byte mutations -- and against the
hand-assembled known answers; and the built library: exported symbols, prototypes at every layer, the pinned ABI constants, is_match and the
header error codes of the two file layers (the walks that need no context), kernel resource notes, the kernel-hash family, the refusal of
Compress."""
import ctypes as C
import gzip
import importlib.util
import json
import os
import random
import re
import subprocess
import sys
import zlib

import pytest

import inflate_ref as R
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_inflate_decode_batch", "alz_inflate_decode_batch_device", "alz_inflate_measure_batch", "alz_inflate_measure_batch_device",
         "alz_zlib_is_match", "alz_gzip_is_match", "alz_zlib_decompress", "alz_gzip_decompress", "alz_zlib_measure", "alz_gzip_measure")
LEVELS = (0, 1, 6, 9)
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)


def kats():
    return json.load(open(os.path.join(GOLDEN, "inflate_kat.json")))["cases"]


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def text_like(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 10))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b" " if rng.random() < 0.9 else b".\n")
    return bytes(out[:n])


def three_type_stream(seed=3):
    """about 600 bytes holding a stored, a fixed and a dynamic block (the dynamic one last), with its plain text"""
    rng = random.Random(seed)
    a, b, c = bytes(rng.randrange(256) for _ in range(150)), text_like(120, seed), text_like(900, seed + 1)
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    s = co.compress(a) + co.flush(zlib.Z_FULL_FLUSH)
    co2 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    s += co2.compress(b) + co2.flush(zlib.Z_FULL_FLUSH)
    s += raw_deflate(c, 9)
    return s, a + b + c


# ---------------------------------------------------------------------------------------------- the reference decoder against the standard library
def test_valid_streams_of_every_level_and_strategy(test_bmp):
    rng = random.Random(11)
    corpus = [text_like(3000, 1), bytes(2500), bytes(rng.randrange(256) for _ in range(1500)), test_bmp[54:54 + 2048], test_bmp[600000:600000 + 3000], b"", b"x"]
    kinds = set()
    for d in corpus:
        for level in LEVELS:
            for strategy in STRATEGIES:
                s = raw_deflate(d, level, strategy)
                kinds.add((s[0] >> 1) & 3)
                tail = bytes(rng.randrange(256) for _ in range(5))
                o = zlib.decompressobj(-15)
                assert o.decompress(s + tail) == d and o.eof
                assert R.decode(s + tail) == (R.OK, d, len(s + tail) - len(o.unused_data)), (len(d), level, strategy)
    assert kinds == {0, 1, 2}


def test_every_prefix_of_three_streams(test_bmp):
    streams = [three_type_stream()[0], raw_deflate(test_bmp[300000:300000 + 1500], 6), raw_deflate(text_like(2000, 5), 1, zlib.Z_FIXED)]
    for k, s in enumerate(streams):
        truncated = 0
        for cut in range(len(s)):
            o = zlib.decompressobj(-15)
            z = o.decompress(s[:cut])
            st, out, used = R.decode(s[:cut])
            assert not o.eof and (st, used) == (R.TRUNC, cut) and len(out) == len(z) and out == z, (k, cut)
            truncated += 1
        assert truncated == len(s) and R.decode(s)[0] == R.OK


def test_single_byte_mutations():
    """zlib.error exactly when the reference decoder says BAD_TOKEN; otherwise the same bytes, and eof exactly when it says OK"""
    rng = random.Random(77)
    bases = [three_type_stream()[0], raw_deflate(text_like(1500, 9), 9), raw_deflate(bytes(rng.randrange(4) for _ in range(1200)), 6)]
    seen = {R.OK: 0, R.TRUNC: 0, R.BAD: 0}
    for i in range(450):
        m = bytearray(bases[i % 3])
        k = rng.randrange(len(m))
        m[k] = m[k] ^ (1 << rng.randrange(8)) if i % 2 else rng.randrange(256)
        o = zlib.decompressobj(-15)
        try:
            z, err = o.decompress(bytes(m)), False
        except zlib.error:
            z, err = None, True
        st, out, used = R.decode(bytes(m))
        assert err == (st == R.BAD), (i, st, err)
        if not err:
            assert out == z and (st == R.OK) == o.eof and st in (R.OK, R.TRUNC), i
            if st == R.OK:
                assert used == len(m) - len(o.unused_data), i
        seen[st] += 1
    assert seen[R.OK] >= 20 and seen[R.BAD] >= 20 and seen[R.TRUNC] >= 1, seen


def test_assembler_round_trips_through_zlib():
    """what the assembler writes, zlib reads: fixed and dynamic blocks with explicit lengths, repeats, a stored block at every bit phase"""
    rng = random.Random(4)
    for t in range(60):
        toks, produced = [], 0
        for _ in range(rng.randrange(1, 80)):
            if produced == 0 or rng.random() < 0.5:
                toks.append(("lit", rng.randrange(256))); produced += 1
            else:
                L = rng.choice([3, 4, 10, 11, 18, 67, 130, 227, 257, 258])
                toks.append(("match", L, min(rng.choice([1, 2, 3, 4, 5, 8, 9, 24, 33, 100, 300]), produced))); produced += L
        w = R.BitWriter()
        R.stored_block(w, b"pre", False)
        R.fixed_block(w, toks[:len(toks) // 2], False)
        lit, dist = R.lens_for(toks)
        R.dynamic_block(w, toks[len(toks) // 2:], True, lit, dist, cl_syms=R.rle_lengths(lit + dist) if t % 2 else None)
        s = w.bytes(fill=t & 1)
        plain = b"pre" + R.expected([("lit", x) for x in b"pre"] + toks)[3:]
        assert zlib.decompressobj(-15).decompress(s) == plain, t
        assert R.decode(s) == (R.OK, plain, len(s)), t


# ---------------------------------------------------------------------------------------------- known answers
def test_kat_file_is_what_its_generator_writes():
    spec = importlib.util.spec_from_file_location("make_inflate_kats_t", os.path.join(GOLDEN, "make_inflate_kats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.CASES == kats()
    names = " | ".join(c["name"] for c in m.CASES)
    for need in ("three literals, a match", "dst_cap inside the match", "cut inside the match", "empty input", "symbol 286", "distance symbol 30",
                 "distance 2 with one byte", "block type 3", "NLEN is not the complement", "LEN 0", "no distance code", "no code for end of block",
                 "runs past the last length", "16 with no previous", "incomplete code-length", "over-subscribed code-length", "HLIT 30", "HDIST 30"):
        assert need in names, need
    src = open(os.path.join(GOLDEN, "make_inflate_kats.py")).read()
    body = src.split('"""')[2]
    assert "inflate_ref" not in body and "zlib" not in body and "import ctypes" not in src          # the generator calls no decoder


@pytest.mark.parametrize("k", range(len(kats())), ids=lambda k: kats()[k]["name"].replace(" ", "_"))
def test_ref_against_kat(k):
    c = kats()[k]
    st, out, used = R.decode(bytes.fromhex(c["src"]), c["cap"])
    assert (st, out.hex(), len(out), used) == (c["status"], c["out"], c["dst_len"], c["src_used"])
    # ... and the standard library agrees on the bytes, and on error / end of stream where the capacity does not cut the stream
    o = zlib.decompressobj(-15)
    try:
        z, err = o.decompress(bytes.fromhex(c["src"])), False
    except zlib.error:
        z, err = None, True
    if c["status"] != R.CAPACITY:
        assert err == (c["status"] == R.BAD) and (err or (z == out and o.eof == (c["status"] == R.OK)))


# ---------------------------------------------------------------------------------------------- the built library
def test_library_exports_the_ten_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _header_protos():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(1): SB._c_param_types(m.group(2)) for m in re.finditer(r"\bint\s+(alz_(?:inflate|zlib|gzip)_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_prototypes_agree_in_header_abi_and_shim():
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert sorted(A.INFLATE_PROTOTYPES) == sorted(NAMES)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"int32_t\*", C.POINTER(C.c_int32)), (r"size_t\*", C.POINTER(C.c_size_t)),
                (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    for name in NAMES:
        want = [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in protos[name]]
        assert A.INFLATE_PROTOTYPES[name] == want, name
        m = re.search(r"\[DllImport\(Lib\)\]\s+internal static extern int %s\(([^)]*)\)" % name, native)
        assert m, name
        cs = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        assert len(cs) == len(protos[name]), name
        for ct, cst in zip(protos[name], cs):
            assert cst == next(w for rx, w in SB.C_TO_CS if re.fullmatch(rx, ct)), (name, ct, cst)
    # the batch entries take what the aPLib twins take
    for kind in ("decode_batch", "decode_batch_device", "measure_batch", "measure_batch_device"):
        assert A.INFLATE_PROTOTYPES["alz_inflate_" + kind] == A.APLIB_PROTOTYPES["alz_aplib_" + kind]
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == A.INFLATE_PROTOTYPES[name]
    from auroralib.compression_amd.batch import Context
    for m in ("inflate_decode_batch", "inflate_decode_batch_device", "inflate_measure_batch", "inflate_measure_batch_device"):
        assert callable(getattr(Context, m))


def test_pinned_abi_constants_are_unchanged():
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text)
    assert re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert (A.ABI_VERSION, A.FMT_COUNT, A.C_COUNT) == (2, 25, 46)
    assert not re.search(r"ALZ_FMT_(DEFLATE|INFLATE|ZLIB|GZIP)|ALZ_C_(DEFLATE|INFLATE|ZLIB|GZIP)", text)
    assert not re.search(r"alz_(aplib|bitlz|crilayla|allz)_\w*(inflate|zlib|gzip)", text)


def test_is_match_on_the_library():
    from auroralib.compression_amd import _lib
    from auroralib.compression_amd import formats as F
    lib = _lib.load()
    z = zlib.compress(b"hello hello hello hello", 6)
    assert z[:2] == b"\x78\x9c" and lib.alz_zlib_is_match(z, len(z)) == 1
    assert lib.alz_zlib_is_match(z[:5], 5) == 1 and lib.alz_zlib_is_match(z[:4], 4) == 0                    # Position + 4 < Length
    for cmf, flg in ((0x78, 0x01), (0x78, 0x5E), (0x78, 0xDA), (0x08, 0x1D), (0x68, 0x81)):
        assert (cmf * 256 + flg) % 31 == 0 and lib.alz_zlib_is_match(bytes([cmf, flg]) + z[2:], len(z)) == 1, (cmf, flg)
    assert lib.alz_zlib_is_match(b"\x79\x9c" + z[2:], len(z)) == 0                                          # CM 9
    assert (0x88 * 256 + 0x1C) % 31 == 0 and lib.alz_zlib_is_match(b"\x88\x1c" + z[2:], len(z)) == 0        # CINFO 8
    assert lib.alz_zlib_is_match(b"\x78\x9d" + z[2:], len(z)) == 0                                          # FCHECK
    assert lib.alz_zlib_is_match(b"\x78\x9c\x07\x00\x00", 5) == 0 and lib.alz_zlib_is_match(b"\x78\x9c\x06\x00\x00", 5) == 0   # block type 3
    # the stored-block test as written: LEN is the first two DATA bytes (header byte included), compared with its own complement, and not 0
    s0 = zlib.compress(b"abc", 0)
    assert s0[2] == 0x01 and lib.alz_zlib_is_match(s0, len(s0)) == 1
    assert lib.alz_zlib_is_match(b"\x78\x01\x00\x00\x00", 5) == 0 and lib.alz_zlib_is_match(b"\x78\x01\x00\x01\x00", 5) == 1
    assert lib.alz_zlib_is_match(b"\x78\x01\x01\x00\x00", 5) == 1
    assert lib.alz_zlib_is_match(None, 0) == 0
    g = gzip.compress(b"hello", mtime=0)
    assert lib.alz_gzip_is_match(g, len(g)) == 1 and lib.alz_gzip_is_match(g[:9], 9) == 1 and lib.alz_gzip_is_match(g[:8], 8) == 0
    assert lib.alz_gzip_is_match(b"\x1f\x8b\x09" + g[3:], len(g)) == 0 and lib.alz_gzip_is_match(b"\x1f\x8c" + g[2:], len(g)) == 0
    assert lib.alz_gzip_is_match(None, 0) == 0
    assert F.ZLib().IsMatch(z) and not F.ZLib().IsMatch(g) and F.GZip().IsMatch(g) and not F.GZip().IsMatch(z)


def _file_rc(fn, data, ctx=None, cap=64):
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    dst = (C.c_uint8 * max(cap, 1))()
    dl, su, st = C.c_size_t(777), C.c_size_t(777), C.c_int32(77)
    if fn.endswith("_measure"):
        rc = getattr(lib, fn)(ctx, data, len(data), cap, C.byref(dl), C.byref(su), C.byref(st))
    else:
        rc = getattr(lib, fn)(ctx, data, len(data), dst, cap, C.byref(dl), C.byref(su), C.byref(st))
    return rc, st.value, dl.value, su.value


def test_header_error_codes_need_no_context():
    z = zlib.compress(b"hello hello", 6)
    for fn in ("alz_zlib_decompress", "alz_zlib_measure"):
        assert _file_rc(fn, b"")[0] == A.E_FORMAT and _file_rc(fn, z[:1])[0] == A.E_FORMAT, fn
        assert _file_rc(fn, b"\x79\x9c" + z[2:])[0] == A.E_FORMAT, fn                                      # CM
        assert _file_rc(fn, b"\x88\x1c" + z[2:])[0] == A.E_FORMAT, fn                                      # CINFO 8
        assert _file_rc(fn, b"\x78\x9d" + z[2:])[0] == A.E_FORMAT, fn                                      # FCHECK
        assert (0x78 * 256 + 0xBB) % 31 == 0 and _file_rc(fn, b"\x78\xbb" + z[2:])[0] == A.E_UNSUPPORTED, fn   # FDICT
        assert _file_rc(fn, z) == (A.E_INVALID, A.ST_OK, 0, 0), fn                                         # a good header: the body needs a context
    g = gzip.compress(b"hello hello", mtime=0)
    hdr = bytearray(g[:10])
    for fn in ("alz_gzip_decompress", "alz_gzip_measure"):
        assert _file_rc(fn, b"")[0] == A.E_FORMAT and _file_rc(fn, b"\x1f")[0] == A.E_FORMAT, fn
        assert _file_rc(fn, b"\x1f\x8c" + g[2:])[0] == A.E_FORMAT and _file_rc(fn, b"\x1f\x8b\x07" + g[3:])[0] == A.E_FORMAT, fn
        for bit in (0x20, 0x40, 0x80):
            assert _file_rc(fn, g[:3] + bytes([bit]) + g[4:])[0] == A.E_FORMAT, (fn, bit)
        for cut in range(2, 10):                                                                           # the fixed part of the header is cut
            assert _file_rc(fn, g[:cut]) == (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0, cut), (fn, cut)
        # FEXTRA whose XLEN runs past the input; FNAME / FCOMMENT without a terminator; FHCRC cut; FHCRC wrong
        h = bytes(hdr[:3]) + b"\x04" + bytes(hdr[4:])
        assert _file_rc(fn, h + b"\x05")[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED) and _file_rc(fn, h + b"\x05\x00abcd")[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), fn
        assert _file_rc(fn, h + b"\xff\xff" + bytes(300))[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), fn
        for flag in (0x08, 0x10, 0x18):
            h = bytes(hdr[:3]) + bytes([flag]) + bytes(hdr[4:])
            assert _file_rc(fn, h + b"name-without-end")[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), (fn, flag)
        h = bytes(hdr[:3]) + b"\x02" + bytes(hdr[4:])
        crc = zlib.crc32(h) & 0xFFFF
        assert _file_rc(fn, h + bytes([crc & 0xFF]))[:2] == (A.E_STREAM, A.ST_INPUT_TRUNCATED), fn
        assert _file_rc(fn, h + bytes([crc & 0xFF, (crc >> 8) ^ 1]) + g[10:])[0] == A.E_CHECKSUM, fn
        assert _file_rc(fn, h + bytes([crc & 0xFF, crc >> 8]) + g[10:])[0] == A.E_INVALID, fn              # a good header: the body needs a context
        assert _file_rc(fn, g)[0] == A.E_INVALID, fn
    from auroralib.compression_amd import _lib
    assert _lib.load().alz_zlib_decompress(None, None, 5, None, 0, None, None, None) == A.E_INVALID


def test_python_classes_refuse_compress_and_stay_outside_all_formats():
    from auroralib.compression_amd import formats as F
    for cls in (F.ZLib, F.GZip):
        with pytest.raises(NotImplementedError) as e:
            cls().Compress(b"abc")
        assert cls.__name__ in str(e.value) and "zlib build" in str(e.value)
        assert cls not in F.ALL_FORMATS
        for m in ("IsMatch", "Decompress", "Compress"):
            assert callable(getattr(cls, m))
    assert F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20] and len(F.ALL_FORMATS) == len(set(F.ALL_FORMATS))


def test_kernel_hash_family():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["inflate"] == ["alz_inflate.hip", "alz_inflate.h"]
    for fam in KH.FAMILIES:
        files = KH.family_files(fam)
        assert ("alz_inflate.hip" in files) == (fam == "inflate") and ("alz_inflate.h" in files) == (fam == "inflate"), fam
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_inflate.hip" in build and "alz_inflate_file.cpp" in build


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_inflate" in n}
    assert len(k) == 2 and sum("alz_inflate_decode_kernel" in n for n in k) == 1 and sum("alz_inflate_measure_kernel" in n for n in k) == 1, sorted(k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] <= 6 * 1024, (n, v)                                           # the LDS budget: at least 24 wavefronts per CU
    assert not any("alz_aplib" in n or "alz_bitlz" in n or "alz_measure_" in n for n in k)
