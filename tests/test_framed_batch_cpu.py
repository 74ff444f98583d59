"""No GPU: the XXH32 family (alz_xxh32_batch*) and the batched LZ4 / Snappy file layer (alz_framed_*) as far as a machine without a device
can hold them: exported symbols, prototypes at every layer (header, _abi tables, loaded argtypes, the shim's [DllImport] lines), the Python
surface, the refusals that need no context, the kernel-hash families, the build list and the kernels' resource notes."""
import ctypes as C
import os
import re
import subprocess
import sys

import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
CSRC = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
NAMES = ("alz_xxh32_batch", "alz_xxh32_batch_device", "alz_framed_decode_batch", "alz_framed_measure_batch")


def lib():
    from auroralib.compression_amd import _lib
    return _lib.load()


def test_library_exports_the_four_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _header_protos():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(2): (m.group(1), SB._c_param_types(m.group(3)))
            for m in re.finditer(r"\b(int|uint32_t)\s+(alz_(?:xxh32|framed)_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_prototypes_agree_in_header_abi_library_and_shim():
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert sorted(A.XXH32_PROTOTYPES) == sorted(n for n in NAMES if "xxh32" in n) and sorted(A.FRAMED_PROTOTYPES) == sorted(n for n in NAMES if "framed" in n)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_file_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    cs_of = SB.C_TO_CS + [(r"alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    table = {**A.XXH32_PROTOTYPES, **A.FRAMED_PROTOTYPES}
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int", name
        assert table[name] == [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in params], name
        fn = getattr(lib(), name)
        assert fn.argtypes == table[name] and fn.restype is C.c_int, name
        m = re.search(r"\[DllImport\(Lib(?:, ExactSpelling = true)?\)\]\s+internal static extern (\w+) %s\(([^)]*)\)" % name, native)
        assert m and m.group(1) == "int", name
        cs = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        assert len(cs) == len(params), name
        for ct, cst in zip(params, cs):
            assert cst == next(w for rx, w in cs_of if re.fullmatch(rx, ct)), (name, ct, cst)
    # the seed stands where the checksum family has its kind; the framed calls have the argument lists of the zfile calls
    assert A.XXH32_PROTOTYPES["alz_xxh32_batch"] == A.CHECKSUM_PROTOTYPES["alz_checksum_batch"]
    assert A.FRAMED_PROTOTYPES["alz_framed_decode_batch"] == A.ZFILE_PROTOTYPES["alz_zfile_decode_batch"]
    assert A.FRAMED_PROTOTYPES["alz_framed_measure_batch"] == A.ZFILE_PROTOTYPES["alz_zfile_measure_batch"]
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert A.FRAMED_CONTAINERS == (A.C_LZ4_FRAME, A.C_LZ4_LEGACY, A.C_SNAPPY) == (22, 7, 9)


def test_the_python_surface_is_there():
    from auroralib.compression_amd.batch import Context
    from auroralib.compression_amd import formats as F
    for m in ("xxh32_batch", "xxh32_batch_device", "framed_decode_batch", "framed_measure_batch"):
        assert callable(getattr(Context, m)), m
    for cls in (F.LZ4, F.LZ4Legacy, F.Snappy):
        assert callable(cls.DecompressMany) and cls.DecompressMany is not getattr(F.ZLib, "DecompressMany"), cls
    assert callable(F.ZLib.DecompressMany) and callable(F.GZip.DecompressMany)
    assert not hasattr(F.LZO, "DecompressMany")                                    # only the classes whose files the batch layer reads


def test_refusals_that_need_no_context():
    L = lib()
    out = (C.c_uint32 * 1)()
    st = (A.Stream * 1)(A.Stream(0, 0, 4, 16, 0, 0, 0, 0))
    buf = (C.c_uint8 * 16)()
    res = (A.FileResult * 1)()
    for seed in (0, 1, 0x9E3779B1, 0xFFFFFFFF):                                    # a NULL context, whatever the seed
        assert L.alz_xxh32_batch(None, seed, 1, buf, 16, st, out) == A.E_INVALID
        assert L.alz_xxh32_batch_device(None, seed, 1, buf, 16, st, out) == A.E_INVALID
        assert L.alz_xxh32_batch(None, seed, 0, None, 0, None, None) == A.E_INVALID
    for fmt in (A.C_LZ4_FRAME, A.C_LZ4_LEGACY, A.C_SNAPPY, 0, 0xFFFFFFFF):         # ... whatever the format
        st[0].format = fmt
        assert L.alz_framed_decode_batch(None, 1, buf, 16, st, buf, 16, res) == A.E_INVALID
        assert L.alz_framed_measure_batch(None, 1, buf, 16, st, res) == A.E_INVALID
        assert L.alz_framed_decode_batch(None, 0, None, 0, None, None, 0, None) == A.E_INVALID


def test_kernel_hash_families_and_build_list():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["xxh32"] == ["alz_xxh32.hip", "alz_xxh32.h"]
    assert KH.FAMILIES["filebatch"] == ["alz_file_batch.h"]
    # no family that was there before lists another file than it did (since then: the encoder's bit-stream section has become a header of its family, alz_encode_bits.h)
    before = {"decode": ["alz_kernels.hip", "alz_big.hip", "alz_decode_fast.h", "alz_decode_serial.h", "alz_device.h", "alz_emit_byte.h", "alz_emit_chunk.h", "alz_prs_table.h", "alz_internal.h"],
              "encode": ["alz_encode.hip", "alz_encode_big.h", "alz_encode_bits.h", "alz_encode_seg.h", "alz_encode_seg_seq.h", "alz_device.h", "alz_internal.h"],
              "measure": ["alz_measure.hip", "alz_measure.h"], "rlh": ["alz_rlh.hip", "alz_rlh.h"], "aplib": ["alz_aplib.hip", "alz_aplib.h"],
              "bitlz": ["alz_bitlz.hip", "alz_bitlz.h"], "inflate": ["alz_inflate.hip", "alz_inflate.h"], "checksum": ["alz_checksum.hip", "alz_checksum.h"],
              "zfile": ["alz_zfile.h"], "framing": ["alz_framing.h"]}
    assert {k: v for k, v in KH.FAMILIES.items() if k in before} == before and sorted(KH.FAMILIES) == sorted(list(before) + ["xxh32", "filebatch"])
    new = {"alz_xxh32.hip": "xxh32", "alz_xxh32.h": "xxh32", "alz_file_batch.h": "filebatch"}
    for fam in KH.FAMILIES:
        files = KH.family_files(fam)
        assert files == sorted(KH.FAMILIES[fam]), (fam, files)                     # every csrc header and kernel file is in a list: nothing is hashed into all
        for f, home in new.items():
            assert (f in files) == (fam == home), (fam, f)
    for fam in ("decode", "encode"):
        for name in KH.FILES:
            assert KH.recorded(name).get(fam) == KH.kernel_hash(fam), (name, fam)  # the committed counters are not made stale
    build = open(os.path.join(CSRC, "build.sh")).read()
    assert "alz_xxh32.hip" in build and "alz_framed_batch.cpp" in build
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in list(new) + ["alz_framed_batch.cpp"])
    unroll = re.search(r"#define ALZ_XXH32_UNROLL (\d+)u", open(os.path.join(CSRC, "alz_xxh32.h")).read())
    assert unroll and int(unroll.group(1)) == 4                                    # tests/test_gpu_xxh32.py puts its lengths around 16 x this


def test_the_batch_layer_is_host_code_on_the_public_abi():
    text = open(os.path.join(CSRC, "alz_framed_batch.cpp")).read()
    assert not re.search(r"\bhip[A-Z]\w+\(|<<<|__global__", text)                  # no HIP call, no launch, no kernel
    assert re.findall(r'#include "([^"]+)"', text) == ["auroralz.h", "alz_file_batch.h", "alz_framing.h", "alz_xxh32.h"]
    zfile = open(os.path.join(CSRC, "alz_zfile.cpp")).read()
    assert '"alz_file_batch.h"' in zfile and "int download(" not in zfile         # one download for both file layers
    container = open(os.path.join(CSRC, "alz_container.cpp")).read()
    assert "lz4_block_reaches_back(" in container and "bool lz4_block_reaches_back" not in container   # ... and one walk over a block's sequences
    assert "inline bool lz4_block_reaches_back" in open(os.path.join(CSRC, "alz_framing.h")).read()


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_xxh32" in n or "alz_range_copy" in n}
    assert len(k) == 2 and sum("alz_xxh32_kernel" in n for n in k) == 1 and sum("alz_range_copy_kernel" in n for n in k) == 1, sorted(k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
        assert v["group_segment_fixed_size"] == 0, (n, v)                          # no LDS, no table
    assert not any("alz_checksum" in n for n in k)
