"""No GPU: CRC-32C of byte ranges (alz_crc32c_batch*, alz_crc32c_combine) and the batched LZ4 / Snappy file WRITER
(alz_framing_compress_batch) as far as a machine without a device can hold them: exported symbols, prototypes at every layer (header, _abi
tables, loaded argtypes, the shim's [DllImport] lines), the Python surface, the refusals that need no context, alz_crc32c_combine against
the oracle, the two new kernels' resource notes, a host model of the chunk kernel's lane arithmetic under the sanitizers, the writers' rules
of csrc/alz_framing.h against the byte-wise model of tests/framing_cases.py, and where the new code lives."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import framing_cases as FC
import oracle_lib as O
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
CSRC = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
NAMES = ("alz_crc32c_batch", "alz_crc32c_batch_device", "alz_crc32c_combine", "alz_framing_compress_batch")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def lib():
    from auroralib.compression_amd import _lib
    return _lib.load()


def test_library_exports_the_four_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def test_prototypes_agree_in_header_abi_library_and_shim():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), SB._c_param_types(m.group(3)))
              for m in re.finditer(r"\b(int|uint32_t)\s+(alz_(?:crc32c|framing)_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(protos) == sorted(NAMES)
    assert sorted(A.CRC32C_PROTOTYPES) == sorted(n for n in NAMES if "crc32c" in n) and list(A.FRAMING_COMPRESS_PROTOTYPES) == ["alz_framing_compress_batch"]
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_settings\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_file_result\*", C.c_void_p),
                (r"(?:const )?uint8_t\*", C.c_void_p), (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"uint32_t", C.c_uint32), (r"uint64_t", C.c_uint64), (r"size_t", C.c_size_t)]
    cs_of = SB.C_TO_CS + [(r"alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    table = {**A.CRC32C_PROTOTYPES, **A.FRAMING_COMPRESS_PROTOTYPES}
    for name in NAMES:
        ret, params = protos[name]
        assert ret == ("uint32_t" if name == "alz_crc32c_combine" else "int"), name
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
    # the CRC-32C batch is the checksum batch without its kind; the writer has the argument list of the decode batch behind the settings
    ck = A.CHECKSUM_PROTOTYPES["alz_checksum_batch"]
    assert A.CRC32C_PROTOTYPES["alz_crc32c_batch"] == ck[:1] + ck[2:] == A.CRC32C_PROTOTYPES["alz_crc32c_batch_device"]
    fd = A.FRAMED_PROTOTYPES["alz_framed_decode_batch"]
    assert A.FRAMING_COMPRESS_PROTOTYPES["alz_framing_compress_batch"] == fd[:1] + [C.c_void_p] + fd[1:]
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert "ALZ_CK_CRC32C" not in text                                             # not a public kind: alz_checksum_batch keeps refusing 2


def test_the_python_surface_is_there():
    from auroralib.compression_amd.batch import Context
    from auroralib.compression_amd import formats as F
    for m in ("crc32c_batch", "crc32c_batch_device", "framing_compress_batch"):
        assert callable(getattr(Context, m)), m
    for cls in (F.LZ4, F.LZ4Legacy, F.Snappy):
        assert callable(cls.CompressMany), cls
    assert not hasattr(F.LZO, "CompressMany") and not hasattr(F.ZLib, "CompressMany")   # only the classes whose files the batch layer writes


def test_refusals_that_need_no_context():
    L = lib()
    out = (C.c_uint32 * 1)(7)
    st = (A.Stream * 1)(A.Stream(0, 0, 4, 16, 0, 0, 0, 0))
    buf = (C.c_uint8 * 16)()
    res = (A.FileResult * 1)()
    assert L.alz_crc32c_batch(None, 1, buf, 16, st, out) == A.E_INVALID
    assert L.alz_crc32c_batch_device(None, 1, buf, 16, st, out) == A.E_INVALID
    assert L.alz_crc32c_batch(None, 0, None, 0, None, None) == A.E_INVALID
    assert out[0] == 7
    settings = A.Settings(8, 0, 0, 0)
    for fmt in (A.C_LZ4_FRAME, A.C_LZ4_LEGACY, A.C_SNAPPY, 0, 0xFFFFFFFF):         # a NULL context, whatever the format
        st[0].format = fmt
        assert L.alz_framing_compress_batch(None, C.byref(settings), 1, buf, 16, st, buf, 16, res) == A.E_INVALID
        assert L.alz_framing_compress_batch(None, None, 1, buf, 16, st, buf, 16, res) == A.E_INVALID
        assert L.alz_framing_compress_batch(None, None, 0, None, 0, None, None, 0, None) == A.E_INVALID
    for kind in (2, 3):                                                            # the launcher's third kind is not a public one
        assert L.alz_checksum_batch(None, kind, 1, buf, 16, st, out) == A.E_INVALID
        assert L.alz_checksum_combine(kind, 1, 2, 3) == 0


def test_combine_against_the_oracle():
    L = lib()
    rng = random.Random(3720)
    big = rng.randbytes(100001 + 70)
    assert O.crc32c(b"123456789") == 0xE3069283 == FC.crc32c_py(b"123456789")
    whole = {}
    for la in range(0, 71):                                                        # pieces of 0 to 70 bytes, every pair of lengths
        for lb in range(0, 71):
            off = (la * 71 + lb) % 50
            a, b = big[off:off + la], big[off + la:off + la + lb]
            key = (off, la + lb)
            if key not in whole:
                whole[key] = O.crc32c(big[off:off + la + lb])
            assert L.alz_crc32c_combine(O.crc32c(a), O.crc32c(b), lb) == whole[key], (la, lb)
    long = big[70:70 + 100001]                                                     # ... and one of 100 001 bytes, on either side
    for short in (b"", big[:1], big[:70]):
        assert L.alz_crc32c_combine(O.crc32c(short), O.crc32c(long), len(long)) == O.crc32c(short + long), len(short)
        assert L.alz_crc32c_combine(O.crc32c(long), O.crc32c(short), len(short)) == O.crc32c(long + short), len(short)
    for v in (0, O.crc32c(b"a"), O.crc32c(long), 0xFFFFFFFF):                      # len_b == 0 is the identity
        assert L.alz_crc32c_combine(v, O.crc32c(b""), 0) == v
    # the length counts modulo nothing smaller than what 64 bits hold: 2^32 + 5 zero bytes behind "abc", joined two ways
    part = O.crc32c(bytes(1 << 16))
    for k in range(16):                                                            # doubling: 2^16 -> 2^32 zero bytes
        part = L.alz_crc32c_combine(part, part, 1 << (16 + k))
    abc, five = O.crc32c(b"abc"), O.crc32c(bytes(5))
    assert L.alz_crc32c_combine(abc, L.alz_crc32c_combine(part, five, 5), (1 << 32) + 5) == L.alz_crc32c_combine(L.alz_crc32c_combine(abc, part, 1 << 32), five, 5)
    # CRC-32 is what it was
    import zlib
    assert L.alz_checksum_combine(A.CK_CRC32, zlib.crc32(big[:999]), zlib.crc32(big[999:5000]), 4001) == zlib.crc32(big[:5000])
    assert L.alz_checksum_combine(A.CK_ADLER32, zlib.adler32(big[:999]), zlib.adler32(big[999:5000]), 4001) == zlib.adler32(big[:5000])


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_crc32c" in n}
    assert len(k) == 2 and sum("alz_crc32c_chunk_kernel" in n for n in k) == 1 and sum("alz_crc32c_fold_kernel" in n for n in k) == 1, sorted(k)
    assert not any("alz_checksum" in n for n in k)                                 # kernels of their own: wrappers, not instantiations of the checksum templates
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)                          # table-free multiplies: no LDS


def _build(tmp_path, name, flags=()):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, "-o", str(exe), os.path.join(ROOT, "tests", name + ".cpp")])
    return str(exe)


def test_host_model_of_the_chunk_kernels_lane_arithmetic(tmp_path):
    """aligned granules, masked head and tail, the per-lane multiply, the table of x^(8 i), x^-120 and the fold, over the helpers of
    csrc/alz_checksum.h for both polynomials: every length up to 200 at every offset 0..15 and the lengths around one and two chunks; every
    load checked against the range, the program built with the address and undefined-behaviour sanitizers and started directly"""
    exe = _build(tmp_path, "crc_lane_model", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    m = re.search(r"(\d+) cases, (\d+) loads, 0 bad", out.stdout)
    assert m and int(m.group(1)) == 2 * (201 * 16 + 6 * 3) + 1 and int(m.group(2)) > 100000


def _lines(tmp_path):
    out = subprocess.run([_build(tmp_path, "framing_write_check")], capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        tag, _, rest = line.partition(" ")
        got.setdefault(tag, []).append(rest.split())
    return got


def _src(off, k):
    return bytes((i * 7 + 3) & 0xFF for i in range(off, off + k))


def _slot(block, k):
    return bytes((block * 31 + j * 5 + 1) & 0xFF for j in range(k))


def _mask(crc):
    return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def test_writer_rules_against_the_python_model(tmp_path):
    g = _lines(tmp_path)
    # descriptor and header checksum byte for the four block sizes (0: the default), none for a size the format does not have
    want_bd = {0: (0x70, 0x400000), 0x10000: (0x40, 0x10000), 0x40000: (0x50, 0x40000), 0x100000: (0x60, 0x100000), 0x400000: (0x70, 0x400000)}
    assert len(g["descriptor"]) == 7
    for opt, bd, block, *rest in g["descriptor"]:
        opt, bd, block = int(opt, 16), int(bd, 16), int(block, 16)
        if opt in want_bd:
            assert (bd, block) == want_bd[opt], hex(opt)
            assert bytes.fromhex(rest[0]) == FC.lz4_frame([], O.xxh32, flg=0x40, bd=bd)[:7], hex(opt)
        else:
            assert bd == 0 and not rest, hex(opt)
    # a compressed and a stored block word, EndMark, the legacy end flag
    assert g["word"] == [["%08x" % 1234, "%08x" % (0x10000 | 0x80000000), "00000000", "ff"]]
    # Snappy chunk headers: type, u24 length with the CRC counted, the CRC masked
    crc9 = FC.crc32c_py(b"123456789")
    assert bytes.fromhex(g["chunk"][0][0]) == bytes([0]) + (304).to_bytes(3, "little") + struct.pack("<I", _mask(crc9))
    assert bytes.fromhex(g["chunk"][1][0]) == bytes([1]) + (0x10004).to_bytes(3, "little") + struct.pack("<I", _mask(0x12345678))
    assert g["errors"] == [[str(A.E_NOMEM), str(A.E_INVALID), str(A.E_INVALID), str(A.E_INVALID)]]
    assert g["slot"] == [[str((0x10000 + 0x4000 + 64 + 255) & ~255), str((0x800000 + 0x200000 + 64 + 255) & ~255)]]
    # refused beforehand: capacity floor first, then the block size, then a last block of 1 to 4 bytes (of the frame's own block size); legacy ignores the option
    assert g["open"] == [[str(v) for v in (A.E_NOMEM, A.E_NOMEM, A.E_INVALID, A.E_INVALID, 0, 0, A.E_INVALID, A.E_NOMEM, 0)]]
    # whole files from made-up block results
    n = 2 * 65536 + 100
    frame = FC.lz4_frame([_src(0, 65536), _slot(1, 500), _slot(2, 60)], O.xxh32, flg=0x40, bd=0x40, raw_flags=[True, False, False])
    assert g["frame"] == [["0", str(len(frame)), "0"]] and bytes.fromhex(g["frame_bytes"][0][0]) == frame
    assert g["frame_caps"] == [["0", str(A.E_NOMEM)]] and g["frame_errors"] == [[str(A.E_NOMEM), str(A.E_INVALID)]]
    legacy = FC.lz4_legacy([_slot(0, 777)])
    assert g["legacy"] == [["0", str(len(legacy)), "0", "800000"]] and bytes.fromhex(g["legacy_bytes"][0][0]) == legacy
    assert g["legacy_caps"] == [["0", str(A.E_NOMEM)]]
    snappy = bytes([0xff, 0x06, 0x00, 0x00]) + b"sNaPpY"
    for i, (stored, body) in enumerate(((True, _src(0, 65536)), (False, _slot(1, 500)), (True, _src(2 * 65536, 100)))):
        snappy += bytes([1 if stored else 0]) + (len(body) + 4).to_bytes(3, "little") + struct.pack("<I", _mask(0x01010101 * (i + 1))) + body
    assert g["snappy"] == [["0", str(len(snappy)), "0"]] and bytes.fromhex(g["snappy_bytes"][0][0]) == snappy
    assert g["snappy_caps"] == [["0", str(A.E_NOMEM)]] and g["snappy_empty"] == [["0", "10"]]
    assert n == 131172


def test_one_copy_of_the_rules_and_where_the_code_lives():
    container = open(os.path.join(CSRC, "alz_container.cpp")).read()
    batch = open(os.path.join(CSRC, "alz_framing_compress.cpp")).read()
    framing = open(os.path.join(CSRC, "alz_framing.h")).read()
    for rule in ("lz4_write_open", "lz4_write_blocks", "snappy_write_open", "snappy_write_chunks"):
        assert "inline int %s(" % rule in framing and rule + "(" in container and rule + "(" in batch, rule
    for once in ("snappy_crc_mask", "0x80000000u", "kLz4EndMark", "xxh32(out + 4, 2, 0)"):   # the mask, the stored bit, the EndMark and the header checksum byte: written once
        assert once in framing and once not in batch, once
    assert "snappy_crc_mask" not in container and "0x80000000u" not in container.split("lz4_file_compress")[1].split("snappy_in_order")[0]
    assert not re.search(r"\bhip[A-Z]\w+\(|<<<|__global__", batch)                # host code on the public ABI: no HIP call, no launch, no kernel
    assert "alz_encode_batch_device(" in batch and "alz_crc32c_batch_device(" in batch and "alz_host_range_copy(" in batch and "download(" in batch
    hip = open(os.path.join(CSRC, "alz_checksum.hip")).read()
    assert "__global__ __launch_bounds__(256) void alz_crc32c_chunk_kernel" in hip and "__global__ __launch_bounds__(64) void alz_crc32c_fold_kernel" in hip
    assert "alz_framing_compress.cpp" in open(os.path.join(CSRC, "build.sh")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_framing_compress.py"))
