"""No GPU: the checksum family (alz_checksum_batch*, alz_checksum_combine) and the batched ZLib / GZip file layer (alz_zfile_*) as far as a
machine without a device can hold them: exported symbols, prototypes at every layer (header, _abi tables, loaded argtypes, the shim's
[DllImport] lines -- with a type mapping of its own, because three of the five carry types tests/test_shim_binding.py has no mapping for),
the size of alz_file_result in C, alz_checksum_combine against the standard library's zlib, the refusals that need no context, the
kernels' resource notes, the kernel-hash families and the build list."""
import ctypes as C
import os
import random
import re
import subprocess
import sys
import zlib

import pytest

import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_checksum_batch", "alz_checksum_batch_device", "alz_checksum_combine", "alz_zfile_decode_batch", "alz_zfile_measure_batch")
REF = {A.CK_ADLER32: zlib.adler32, A.CK_CRC32: zlib.crc32}


def lib():
    from auroralib.compression_amd import _lib
    return _lib.load()


def test_library_exports_the_five_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _header_protos():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(2): (m.group(1), SB._c_param_types(m.group(3)))
            for m in re.finditer(r"\b(int|uint32_t)\s+(alz_(?:checksum|zfile)_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_prototypes_agree_in_header_abi_library_and_shim():
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert sorted(list(A.CHECKSUM_PROTOTYPES) + list(A.ZFILE_PROTOTYPES)) == sorted(NAMES)
    assert sorted(A.CHECKSUM_PROTOTYPES) == sorted(n for n in NAMES if "checksum" in n)
    assert not any(n in A.INFLATE_PROTOTYPES for n in NAMES) and len(A.INFLATE_PROTOTYPES) == 10
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_file_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"uint32_t", C.c_uint32), (r"uint64_t", C.c_uint64), (r"size_t", C.c_size_t)]
    cs_of = SB.C_TO_CS + [(r"alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    table = {**A.CHECKSUM_PROTOTYPES, **A.ZFILE_PROTOTYPES}
    for name in NAMES:
        ret, params = protos[name]
        assert ret == ("uint32_t" if name == "alz_checksum_combine" else "int"), name
        assert table[name] == [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in params], name
        fn = getattr(lib(), name)
        assert fn.argtypes == table[name], name
        assert fn.restype is (C.c_uint32 if ret == "uint32_t" else C.c_int), name
        m = re.search(r"\[DllImport\(Lib(?:, ExactSpelling = true)?\)\]\s+internal static extern (\w+) %s\(([^)]*)\)" % name, native)
        assert m and m.group(1) == ("uint" if ret == "uint32_t" else "int"), name
        cs = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        assert len(cs) == len(params), name
        for ct, cst in zip(params, cs):
            assert cst == next(w for rx, w in cs_of if re.fullmatch(rx, ct)), (name, ct, cst)
    from auroralib.compression_amd.batch import Context
    from auroralib.compression_amd import formats as F
    for m in ("checksum_batch", "checksum_batch_device", "zfile_decode_batch", "zfile_measure_batch"):
        assert callable(getattr(Context, m))
    assert callable(F.ZLib.DecompressMany) and callable(F.GZip.DecompressMany)


def test_constants_and_the_result_struct_match_the_c_abi(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "auroralz.h"\nint main(void){printf("%zu %zu %zu %zu %zu %u %u %u %u\\n", sizeof(alz_file_result), '
                    "offsetof(alz_file_result, rc), offsetof(alz_file_result, status), offsetof(alz_file_result, dst_len), offsetof(alz_file_result, src_used), "
                    "(unsigned)ALZ_CK_ADLER32, (unsigned)ALZ_CK_CRC32, ALZ_ZFILE_ZLIB, ALZ_ZFILE_GZIP);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [16, 0, 4, 8, 12, 0, 1, 0, 1]
    assert C.sizeof(A.FileResult) == 16 and [(f, getattr(A.FileResult, f).offset) for f, _ in A.FileResult._fields_] == [("rc", 0), ("status", 4), ("dst_len", 8), ("src_used", 12)]
    assert (A.CK_ADLER32, A.CK_CRC32, A.ZFILE_ZLIB, A.ZFILE_GZIP) == (0, 1, 0, 1)
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    m = re.search(r"\[StructLayout\(LayoutKind\.Sequential, Size = 16\)\]\s*public struct AlzFileResult\s*\{(.*?)\n    \}", native, flags=re.S)
    assert m and re.findall(r"public (\w+) (\w+);", m.group(1)) == [("int", "Rc"), ("int", "Status"), ("uint", "DstLen"), ("uint", "SrcUsed")]
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)


def _combine(kind, a, b, n):
    return lib().alz_checksum_combine(kind, a, b, n)


@pytest.mark.parametrize("kind", (A.CK_ADLER32, A.CK_CRC32), ids=("adler32", "crc32"))
def test_combine_against_zlib(kind):
    ref = REF[kind]
    rng = random.Random(1950 + kind)
    big = rng.randbytes((1 << 20) + 70000)
    ff = b"\xff" * ((1 << 20) + 70000)
    for t in range(1000):                                                          # random splits of random buffers up to 1 MiB
        n = rng.choice((rng.randrange(0, 64), rng.randrange(0, 70000), rng.randrange(0, (1 << 20) + 1)))
        off = rng.randrange(0, (1 << 20) - n + 1)
        cut = rng.randrange(0, n + 1)
        a, b = big[off:off + cut], big[off + cut:off + n]
        assert _combine(kind, ref(a), ref(b), len(b)) == ref(big[off:off + n]), (t, n, cut)
    for src in (big, ff):
        for len_b in (0, 1, 5552, 5553, 65521, 1 << 20):
            for len_a in (0, 1, 5553, 65521):
                a, b = src[:len_a], src[len_a:len_a + len_b]
                assert len(b) == len_b and _combine(kind, ref(a), ref(b), len_b) == ref(a + b), (len_a, len_b)
    for v in (ref(b""), ref(b"a"), ref(ff), ref(big)):                             # len_b == 0 is the identity
        assert _combine(kind, v, ref(b""), 0) == v
    # the length counts modulo nothing smaller than what 64 bits hold: B of 2^32 + 5 zero bytes, joined from two halves of known sums
    half = ref(bytes(1 << 16))
    whole = half
    for k in range(16):                                                            # doubling: 2^16 -> 2^32 zero bytes
        n = 1 << (16 + k)
        whole = _combine(kind, whole, whole, n)
    assert _combine(kind, ref(b"abc"), _combine(kind, whole, ref(bytes(5)), 5), (1 << 32) + 5) == _combine(kind, _combine(kind, ref(b"abc"), whole, 1 << 32), ref(bytes(5)), 5)
    assert _combine(7, 1, 2, 3) == 0                                               # an unknown kind


def test_refusals_that_need_no_context():
    L = lib()
    out = (C.c_uint32 * 1)()
    st = (A.Stream * 1)(A.Stream(0, 0, 4, 16, 0, 0, 0, 0))
    buf = (C.c_uint8 * 16)()
    res = (A.FileResult * 1)()
    for kind in (0, 1, 2, 77):                                                     # a NULL context, whatever the kind
        assert L.alz_checksum_batch(None, kind, 1, buf, 16, st, out) == A.E_INVALID
        assert L.alz_checksum_batch_device(None, kind, 1, buf, 16, st, out) == A.E_INVALID
        assert L.alz_checksum_batch(None, kind, 0, None, 0, None, None) == A.E_INVALID
    for fmt in (0, 1, 2, 0xFFFFFFFF):                                              # ... whatever the format
        st[0].format = fmt
        assert L.alz_zfile_decode_batch(None, 1, buf, 16, st, buf, 16, res) == A.E_INVALID
        assert L.alz_zfile_measure_batch(None, 1, buf, 16, st, res) == A.E_INVALID


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_checksum" in n}
    assert len(k) == 4 and sum("alz_checksum_chunk_kernel" in n for n in k) == 2 and sum("alz_checksum_fold_kernel" in n for n in k) == 2, sorted(k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)                          # table-free: no LDS either
    assert not any("alz_inflate" in n for n in k)


def test_kernel_hash_families_and_build_list():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["checksum"] == ["alz_checksum.hip", "alz_checksum.h"]
    assert KH.FAMILIES["zfile"] == ["alz_zfile.h"]
    new = ("alz_checksum.hip", "alz_checksum.h", "alz_zfile.h")
    for fam in KH.FAMILIES:
        files = KH.family_files(fam)
        for f in new[:2]:
            assert (f in files) == (fam == "checksum"), (fam, f)
        assert ("alz_zfile.h" in files) == (fam == "zfile"), fam
    for fam in ("decode", "encode"):
        assert not any(f in KH.family_files(fam) for f in new), fam
        for name in KH.FILES:
            assert KH.recorded(name).get(fam) == KH.kernel_hash(fam), (name, fam)   # the committed counters are not made stale
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_checksum.hip" in build and "alz_zfile.cpp" in build
    csrc = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
    assert all(os.path.exists(os.path.join(csrc, f)) for f in new + ("alz_zfile.cpp",))
