"""No GPU: the measure entry points (alz_measure_batch, alz_measure_batch_device, alz_container_measure) exist at every layer with matching
arity and types, the built library holds measure kernels for gfx950 that use no scratch and no more registers than the decode kernel of the
same format, and adding them left the decode kernel sources (and with them the recorded counter hash) alone."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alz_measure_batch", "alz_measure_batch_device", "alz_container_measure")
LLVM = "/opt/rocm/lib/llvm/bin"
# the formats with a lane-parallel measure kernel: PRS BE / LE, LZ4 block, LZO, raw Snappy, FastLZ, WFLZ LE / BE
BULK = (A.FMT_PRS_BE, A.FMT_PRS_LE, A.FMT_LZ4_BLOCK, A.FMT_LZO, A.FMT_SNAPPY_RAW, A.FMT_FASTLZ, A.FMT_WFLZ, A.FMT_WFLZ_BE)


def _header_types():
    text = re.sub(r"/\*.*?\*/", " ", open(SB.HDR).read(), flags=re.S)
    return {m.group(2): SB._c_param_types(m.group(3)) for m in re.finditer(r"\b(int)\s+(alz_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_header_declares_the_three_functions_and_keeps_the_abi_version():
    protos = SB._header_prototypes()
    assert {n: protos.get(n) for n in NAMES} == {"alz_measure_batch": 7, "alz_measure_batch_device": 7, "alz_container_measure": 9}
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", open(SB.HDR).read()) and A.ABI_VERSION == 2


def test_python_prototypes_match_the_header():
    """_abi.MEASURE_PROTOTYPES against the header: same arity; pointers as c_void_p (or a typed POINTER), uint32_t / size_t by value."""
    types = _header_types()
    for name in NAMES:
        c, py = types[name], A.MEASURE_PROTOTYPES[name]
        assert len(c) == len(py), name
        for ct, pt in zip(c, py):
            if ct.endswith("*"):
                want = {"size_t*": (C.c_void_p, C.POINTER(C.c_size_t)), "int32_t*": (C.c_void_p, C.POINTER(C.c_int32))}.get(ct, (C.c_void_p,))
                assert pt in want, (name, ct, pt)
            else:
                assert pt is {"uint32_t": C.c_uint32, "size_t": C.c_size_t}[ct], (name, ct, pt)


def test_native_cs_binds_the_three_functions():
    imports, protos = SB._dllimports(), SB._header_prototypes()
    for name in NAMES:
        assert imports.get(name) == protos[name], name          # (the parameter TYPES: test_shim_binding.test_dllimport_parameter_types_match_the_header)
    body = open(os.path.join(SB.SHIM, "AmdBody.cs")).read()
    assert "Native.alz_measure_batch(" in body


def test_library_exports_the_three_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _kernel_notes(tmp_path):
    if not (os.path.exists(LLVM + "/llvm-objdump") and os.path.exists(LLVM + "/llvm-readelf")):
        pytest.skip("no llvm binutils")
    so = shutil.copy(os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so"), tmp_path / "lib.so")
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", str(so)], check=True, capture_output=True, cwd=tmp_path)
    kernels = {}
    for co in tmp_path.glob("lib.so.*gfx950"):
        notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", block)}
    return kernels


def test_measure_kernels_use_no_scratch_and_fewer_registers_than_the_decoder(tmp_path):
    k = _kernel_notes(tmp_path)
    exact = {n: v for n, v in k.items() if "alz_measure_exact_kernel" in n}
    bulk = {n: v for n, v in k.items() if "alz_measure_bulk_kernel" in n}
    assert len(exact) == A.FMT_COUNT and len(bulk) == len(BULK), (sorted(exact), sorted(bulk))
    for n, v in {**exact, **bulk}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
    for fmt in BULK:
        m = [v for n, v in bulk.items() if "alz_measure_bulk_kernelILi%dEE" % fmt in n]
        d = [v for n, v in k.items() if "alz_decode_queue_kernelILi%dEE" % fmt in n]
        assert len(m) == 1 and len(d) == 1, (fmt, m, d)
        print("%s: measure %d VGPRs, decode %d" % (A.FORMAT_NAMES[fmt], m[0]["vgpr_count"], d[0]["vgpr_count"]))
        assert m[0]["vgpr_count"] <= d[0]["vgpr_count"], (A.FORMAT_NAMES[fmt], m[0], d[0])


def test_decode_counter_hash_is_unchanged_and_measure_is_a_family_of_its_own():
    spec = importlib.util.spec_from_file_location("alz_kernel_hash_m", os.path.join(ROOT, "tools", "kernel_hash.py"))
    kh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kh)
    assert sorted(kh.FAMILIES["measure"]) == ["alz_measure.h", "alz_measure.hip"]
    for fam in ("decode", "encode"):
        assert not any(f.startswith("alz_measure") for f in kh.family_files(fam)), fam
        for name in kh.FILES:
            assert kh.recorded(name).get(fam) == kh.kernel_hash(fam), (name, fam)
