"""No GPU: the DEFLATE encoder (alz_deflate_*).  The code builder of csrc/alz_inflate.h -- host and device code -- as a stand-alone program
(tests/deflate_codes_check.cpp), plain and under sanitizers; the token walker against the standard library; and the built library: exported
symbols, prototypes at every layer, the bounds, the refusals that need no context, kernel resource notes, the Python surface."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess
import zlib

import pytest

import deflate_walk as W
import test_inflate_cpu as IC
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
CSRC = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NAMES = ("alz_deflate_bound", "alz_deflate_block_bytes", "alz_deflate_encode_batch", "alz_deflate_encode_batch_device", "alz_deflate_file_bound",
         "alz_deflate_file_compress", "alz_deflate_file_compress_batch")
# the prototypes the existing tests pin, per prefix, as the parent commit has them
PINNED = {"alz_inflate_": 4, "alz_zlib_": 3, "alz_gzip_": 3, "alz_checksum_": 3, "alz_zfile_": 2, "alz_crc32c_": 3, "alz_framing_": 1, "alz_xxh32_": 2, "alz_framed_": 2}


def lib():
    from auroralib.compression_amd import _lib
    return _lib.load()


def _build(tmp_path, flags=()):
    exe = str(tmp_path / ("deflate_codes_check" + ("_san" if flags else "")))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "deflate_codes_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitizers"])
def test_code_builder_as_a_program(tmp_path, flags):
    out = subprocess.run([_build(tmp_path, flags)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    m = re.fullmatch(r"ok (\d+)\n", out.stdout)
    assert m and int(m.group(1)) >= 20000 + 10, out.stdout


def test_walker_reads_what_zlib_writes(test_bmp):
    rng = random.Random(5)
    corpus = [IC.text_like(5000, 1), bytes(3000), bytes(rng.randrange(256) for _ in range(2000)), test_bmp[54:54 + 4096], b"", b"x", b"ab" * 700]
    types = set()
    for d in corpus:
        for level in (0, 1, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE):
                s = IC.raw_deflate(d, level, strategy)
                blocks, used = W.walk(s + b"tail")
                assert used == len(s)
                n = 0
                for b in blocks:
                    types.add(b["type"])
                    assert b["start"] == n
                    n += b["stored"] if b["type"] == W.STORED else sum(1 if t[0] == "lit" else t[1] for t in b["tokens"])
                    assert all(t[0] == "lit" or (3 <= t[1] <= 258 and 1 <= t[2] <= 32768) for t in b["tokens"])
                assert n == len(d) and blocks[-1]["final"] == 1
    assert types == {0, 1, 2}
    s, _ = IC.three_type_stream()
    for bad in (s[:len(s) // 2], b"\x07", bytes([0b101]) + b"\xff\xff"):       # truncated; block type 3; a fixed block of symbols 287
        with pytest.raises(ValueError):
            W.walk(bad)


def test_library_exports_and_prototypes_at_every_layer():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), SB._c_param_types(m.group(3))) for m in re.finditer(r"\b(int|size_t)\s+(alz_deflate_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(protos) == sorted(NAMES) and sorted(A.DEFLATE_PROTOTYPES) == sorted(NAMES)
    assert re.search(r"#define ALZ_DEFLATE_FIXED 1u\b", text) and A.DEFLATE_FIXED == 1
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_result\*|alz_file_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"size_t\*", C.POINTER(C.c_size_t)), (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t), (r"int", C.c_int)]
    cs_of = SB.C_TO_CS + [(r"alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    L = lib()
    for name in NAMES:
        ret, params = protos[name]
        assert A.DEFLATE_PROTOTYPES[name] == [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in params], name
        assert getattr(L, name).argtypes == A.DEFLATE_PROTOTYPES[name] or (not params and not getattr(L, name).argtypes), name
        assert getattr(L, name).restype == (C.c_size_t if ret == "size_t" else C.c_int), name
        m = re.search(r"\[DllImport\(Lib(?:, ExactSpelling = true)?\)\]\s+internal static extern (\w+) %s\(([^)]*)\)" % name, native)
        assert m and m.group(1) == ("UIntPtr" if ret == "size_t" else "int"), name
        cs = [" ".join(p.split()[:-1]) for p in m.group(2).split(",") if p.strip()]
        assert len(cs) == len(params), name
        for ct, cst in zip(params, cs):
            assert cst == next(w for rx, w in cs_of if re.fullmatch(rx, ct)), (name, ct, cst)
    assert A.DEFLATE_PROTOTYPES["alz_deflate_encode_batch"] == A.DEFLATE_PROTOTYPES["alz_deflate_encode_batch_device"] == A.DEFLATE_PROTOTYPES["alz_deflate_file_compress_batch"]


def test_no_prototype_with_a_pinned_prefix_was_added_and_the_constants_stay():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    names = re.findall(r"\b(?:int|void|size_t|uint32_t|uint64_t|const\s+char\s*\*)\s+(alz_\w+)\s*\(", text)
    for prefix, count in PINNED.items():
        assert sum(n.startswith(prefix) for n in names) == count, (prefix, [n for n in names if n.startswith(prefix)])
    full = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", full) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", full) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", full)
    assert not re.search(r"ALZ_FMT_DEFLATE|ALZ_C_DEFLATE", full) and "THERE IS NO ENCODER: the BCL" not in full and "THE ENCODER is alz_deflate_*" in full


def test_bounds():
    L = lib()
    assert L.alz_deflate_block_bytes() >= 4096
    ns = (0, 1, 65535, 65536, 2 ** 31 - 257)
    for kind, extra in ((None, 0), (A.ZFILE_ZLIB, 2 + 4), (A.ZFILE_GZIP, 10 + 8)):
        last = -1
        for n in ns:
            b = L.alz_deflate_bound(n) if kind is None else L.alz_deflate_file_bound(kind, n)
            assert n + extra < b <= n + (n >> 10) + 64 + extra and b > last, (kind, n, b)
            last = b
            if kind is not None:
                assert b == L.alz_deflate_bound(n) + extra
    assert L.alz_deflate_file_bound(2, 100) == 0


def test_refusals_that_need_no_context():
    L = lib()
    st = (A.Stream * 1)(A.Stream(0, 0, 4, 64, 0, 0, 0, 0))
    res, fres = (A.Result * 1)(), (A.FileResult * 1)()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    dl = C.c_size_t(7)
    for level, flags in ((6, 0), (-1, 0), (10, 0), (6, 2)):                    # a NULL context, and with it a bad level, a bad flag
        for fn in ("alz_deflate_encode_batch", "alz_deflate_encode_batch_device"):
            assert getattr(L, fn)(None, level, flags, 1, src, 64, st, dst, 64, res) == A.E_INVALID, (fn, level, flags)
            assert getattr(L, fn)(None, level, flags, 0, None, 0, None, None, 0, None) == A.E_INVALID, (fn, level, flags)
        assert L.alz_deflate_file_compress_batch(None, level, flags, 1, src, 64, st, dst, 64, fres) == A.E_INVALID
        assert L.alz_deflate_file_compress(None, A.ZFILE_GZIP, level, flags, src, 4, dst, 64, C.byref(dl)) == A.E_INVALID and dl.value == 0


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_deflate_" in n}
    assert len(k) == 3 and all(sum(("alz_deflate_%s_kernel" % w) in n for n in k) == 1 for w in ("find", "place", "emit")), sorted(k)
    assert not any("alz_inflate" in n for n in k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] <= 160 * 1024, (n, v)


def test_python_surface_and_deflate_level_tables():
    from auroralib.compression_amd import formats as F
    from auroralib.compression_amd.batch import Context
    for m in ("deflate_encode_batch", "deflate_encode_batch_device", "deflate_file_compress_batch"):
        assert callable(getattr(Context, m))
    for cls in (F.ZLib, F.GZip):
        for m in ("Deflate", "DeflateMany", "DeflateLevel"):
            assert callable(getattr(cls, m))
        with pytest.raises(NotImplementedError) as e:
            cls().Compress(b"abc")
        assert cls.__name__ in str(e.value) and "zlib build" in str(e.value) and "Deflate" in str(e.value)
    gz = {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 1, 7: 6, 8: 6, 9: 6, 10: 9, 11: 9, 12: 9, 13: 9, 14: 9, 15: 9}
    zl = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3, 8: 4, 9: 4, 10: 5, 11: 5, 12: 6, 13: 6, 14: 7, 15: 8}
    for q in range(16):
        for strategy in (0, 1):
            s = F.CompressionSettings(q, 0, strategy)
            assert F.ZLib().DeflateLevel(s) == (zl[q], bool(strategy)) and zl[q] == q * 8 // 15, q
            assert F.GZip().DeflateLevel(s) == (gz[q], False), q


def test_where_the_code_lives():
    build = open(os.path.join(CSRC, "build.sh")).read()
    assert "alz_deflate_file.cpp" in build and os.path.exists(os.path.join(CSRC, "alz_deflate_file.cpp"))
    hip = open(os.path.join(CSRC, "alz_inflate.hip")).read()
    assert len(re.findall(r"__global__[^;{]*?\balz_deflate_\w+_kernel\b", hip, flags=re.S)) == 3
    assert "alz_deflate_plan_block" in open(os.path.join(CSRC, "alz_inflate.h")).read()
    # tools/kernel_hash.py: the family "inflate" is DEFLATE in both directions and no list changed with it (pinned as of the commit that listed
    # alz_encode_bits.h, the encoder's bit-stream section, in the family "encode")
    assert hashlib.sha256(open(os.path.join(ROOT, "tools", "kernel_hash.py"), "rb").read()).hexdigest() == KERNEL_HASH_PY_SHA256


KERNEL_HASH_PY_SHA256 = "ae44c9d7387f02e093040360e5f3833eddd4564a60fd3100a45414de1943a7e3"
