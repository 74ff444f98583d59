"""No GPU: CRILAYLA and ALLZ written (alz_bitenc_*).  The oracle has neither body, so the yardstick of the GPU tests is a Python restatement
(tests/chain_finder_ref.py: LzChainMatchFinder; tests/bitenc_ref.py: the two CompressHeaderless bodies).  Here that restatement is pinned: the
finder under a ten-line LZ10 writer, a Yaz0 writer and -- for the LzProperties[] form -- a RefPack writer must give the oracle's bytes, and the two
restated encoders must round-trip through the restated readers.  Then the built library: exported symbols, prototypes at every layer, the pinned
constants, kernel resource notes, the kernel-hash family."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import pytest

import bitenc_ref as E
import bitlz_ref as R
import chain_finder_ref as CF
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_bitenc_bound", "alz_bitenc_encode_batch", "alz_bitenc_encode_batch_device", "alz_bitenc_file_bound", "alz_bitenc_file_compress",
         "alz_bitenc_file_compress_batch")
LZ10_LZ = CF.LzProperties(0x1000, 18, 3)                                    # LZ10.cs:23
YAZ0_LZ = CF.LzProperties(0x1000, 0xFF + 0x12, 3)                           # Yay0.cs:27
REFPACK_LZ = [CF.LzProperties(0x20000, 1028, 5), CF.LzProperties(0x4000, 67, 4), CF.LzProperties(0x400, 10, 3)]   # RefPack.cs:29-34


# ---------------------------------------------------------------------------------------------- writers that are pure functions of the match list
def lz10_write(data, match_list):        # LZ10.cs:113-137
    fw, sp = CF.FlagWriter(True), 0
    for offset, distance, length in match_list:
        for _ in range(offset - sp):
            fw.buffer.append(data[sp]); fw.write_bit(0); sp += 1
        if length == 0:
            break
        fw.buffer += ((((length - 3) << 12) | ((distance - 1) & 0xFFF)) & 0xFFFF).to_bytes(2, "big")
        sp += length
        fw.write_bit(1)
    fw.flush()
    return bytes(fw.out)


def yaz0_write(data, match_list):        # Yaz0.cs:94-98 over Yay0.cs:152-184
    fw, sp = CF.FlagWriter(True), 0
    for offset, distance, length in match_list:
        for _ in range(offset - sp):
            fw.buffer.append(data[sp]); fw.write_bit(1); sp += 1
        if length == 0:
            break
        if length < 18:
            fw.buffer += (((distance - 1) | ((length - 2) << 12)) & 0xFFFF).to_bytes(2, "big")
        else:
            fw.buffer += ((distance - 1) & 0xFFF).to_bytes(2, "big") + bytes([length - 0x12])
        sp += length
        fw.write_bit(0)
    fw.flush()
    return bytes(fw.out)


def refpack_write(data, match_list):     # RefPack.cs:241-290
    out, sp, plain = bytearray(), 0, 0
    for offset, distance, length in match_list:
        plain = offset - sp
        while plain > 3:
            c = min(plain, 0x70) // 4 - 1
            out.append(0xE0 | c)
            c = c * 4 + 4
            out += data[sp:sp + c]; sp += c; plain -= c
        if length == 0:
            break
        d1 = distance - 1
        if length <= 10 and distance <= 0x400:
            out += bytes([(plain | ((d1 & 0x300) >> 3) | ((length - 3) << 2)) & 0xFF, d1 & 0xFF])
        elif 4 <= length <= 67 and distance <= 0x4000:
            out += bytes([(0x80 | (length - 4)) & 0xFF, ((d1 >> 8) | (plain << 6)) & 0xFF, d1 & 0xFF])
        else:
            out += bytes([(0xC0 | (d1 >> 16 << 4) | ((length - 5) >> 8 << 2) | plain) & 0xFF, (d1 >> 8) & 0xFF, d1 & 0xFF, (length - 5) & 0xFF])
        out += data[sp:sp + plain]
        sp += plain + length
        plain = 0
    out.append(0xFC | plain)
    out += data[sp:sp + plain]
    return bytes(out)


PIN_CASES = [(10240, 0), (10240, 8), (10240, 12), (10240, 15), (65536, 0)]


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib as O
    return O


@pytest.mark.parametrize("size,quality", PIN_CASES)
def test_finder_restatement_gives_the_oracles_lz10_and_yaz0_bytes(test_bmp, oracle, size, quality):
    data = test_bmp[:size]
    assert lz10_write(data, CF.matches(LZ10_LZ, data, quality)) == oracle.encode_stream(A.FMT_LZ10, data, quality)[0]
    assert yaz0_write(data, CF.matches(YAZ0_LZ, data, quality)) == oracle.encode_stream(A.FMT_YAZ0, data, quality)[0]


@pytest.mark.parametrize("size,quality", PIN_CASES)
def test_property_set_form_gives_the_oracles_refpack_bytes(test_bmp, oracle, size, quality):
    data = test_bmp[:size]
    assert refpack_write(data, CF.matches(REFPACK_LZ, data, quality)) == oracle.encode_stream(A.FMT_REFPACK, data, quality)[0]


def test_finder_restatement_on_degenerate_inputs(oracle):
    """runs, short periods and the ends of the buffer, where the lazy step, the fill loop and `limit` meet; the min-length table from quality 10 on"""
    rng = random.Random(5)
    inputs = [b"", b"a", b"abc", b"abcd", bytes(300), b"abc" * 200, bytes(rng.randrange(4) for _ in range(3000)), bytes(rng.randrange(256) for _ in range(2000)) * 2]
    for data in inputs:
        for q in (0, 1, 2, 5, 9, 10, 15):
            assert lz10_write(data, CF.matches(LZ10_LZ, data, q)) == oracle.encode_stream(A.FMT_LZ10, data, q)[0], (len(data), q)
            assert refpack_write(data, CF.matches(REFPACK_LZ, data, q)) == oracle.encode_stream(A.FMT_REFPACK, data, q)[0], (len(data), q)


def test_min_distance_of_the_finder_against_the_oracles_blz(oracle):
    """BLZ's finder has minDistance 3 like CRILAYLA's: skipped candidates use up attempts, the min-table fallback clamps.  Same match list for LZ10's
    geometry with that minimum distance: the oracle's LZ10 body at min_distance 3."""
    lz = CF.LzProperties(0x1000, 18, 3, 0, 3)
    rng = random.Random(9)
    for data in (bytes(500), b"ab" * 300, b"abc" * 300, bytes(rng.randrange(3) for _ in range(4000))):
        for q in (0, 2, 8, 12):
            assert lz10_write(data, CF.matches(lz, data, q)) == oracle.encode_stream(A.FMT_LZ10, data, q, min_distance=3)[0], (len(data), q)


# ---------------------------------------------------------------------------------------------- the restated encoders
def _inputs(test_bmp):
    rng = random.Random(11)
    return [b"", b"x", b"xy", bytes(7), bytes(1000), b"abc" * 400, bytes(rng.randrange(256) for _ in range(1500)),
            bytes(rng.randrange(5) for _ in range(5000)), test_bmp[:10240], test_bmp[0x36:0x36 + 9000]]


def test_restated_crilayla_round_trips(test_bmp):
    for data in _inputs(test_bmp):
        for q in (0, 2, 8, 12):
            body = E.cri_compress_headerless(data, q)
            out, status, n, used = R.cri_decode(body, len(data))
            assert (status, n, out, used) == (R.OK, len(data), data, len(body)), (len(data), q)
    data = test_bmp[:3000]
    f = E.cri_compress(data, 8)
    assert f[:8] == b"CRILAYLA" and int.from_bytes(f[8:12], "little") == len(data) - 0x100 and f[-0x100:] == data[:0x100]
    assert R.cri_file_decode(f)[:3] == ("ok", R.OK, data)
    with pytest.raises(ValueError):
        E.cri_compress(bytes(0xFF))
    # equal bytes at quality 0: distances 1 and 2 use up the one attempt -- no match at all, nine bits per byte
    assert len(E.cri_compress_headerless(bytes(800), 0)) == 900
    assert len(E.cri_compress_headerless(bytes(800), 2)) < 20


def test_restated_allz_round_trips(test_bmp):
    for data in _inputs(test_bmp):
        for q in (0, 2, 8, 12):
            for triple in ((0, 10, 1), (0, 0, 0), (2, 8, 3), (5, 14, 2)):
                body = E.allz_compress_headerless(data, q, *triple)
                out, status, n, used = R.allz_decode(body, len(data), None, *triple)
                assert (status, n, out) == (R.OK, len(data), data), (len(data), q, triple)
                assert used in (len(body), len(body) - 1), (len(data), q, triple)   # (the lone 1-bit behind a final match may open a flag byte the reader never fetches)
    assert E.allz_compress_headerless(b"", 8) == b"\x01"                     # the lone 1-bit  ALLZ.cs:147-153
    f = E.allz_compress(test_bmp[:2000], 8, 2, 8, 3)
    assert f[:8] == b"ALLZ" + bytes([0, 2, 8, 3]) and int.from_bytes(f[8:12], "little") == 2000


def test_allz_tiers_in_the_restated_finder():
    """ScoreMatch takes the first of the five sets that admits a candidate: a repeat at distance D needs 3 / 4 / 5 / 6 / 8 bytes for D up to 0x1000 / 0x4000 /
    0x8000 / 0x20000 / 0x80000, and nothing is taken beyond 0x80000.  (Three bytes are only ever found through the min-length table, from quality 10
    on: the chain hashes four.)"""
    def planted(dist, length, quality=8):            # (quality 8: 24 candidates per search, so that a colliding hash does not hide the planted one)
        filler = bytearray(dist + 66)
        for c in range(len(filler) // 3):            # (an 18-bit counter, six bits per byte, the byte's place in its top two bits: no three bytes repeat, wherever they start)
            filler[3 * c:3 * c + 3] = bytes([0x80 | c & 0x3F, 0x40 | (c >> 6) & 0x3F, (c >> 12) & 0x3F])
        data = bytes(filler[:dist]) + bytes(filler[:length]) + b"\xFE\xFD\xFC\xFB\xFA"
        return [m for m in CF.matches(E.ALLZ_LZ, data, quality) if m[2]]
    assert planted(0x1000, 3, 10) == [(0x1000, 0x1000, 3)] and planted(0x1001, 3, 10) == []
    assert planted(0x1000, 4) == [(0x1000, 0x1000, 4)] and planted(0x1001, 4) == [(0x1001, 0x1001, 4)]
    assert planted(0x4000, 4) == [(0x4000, 0x4000, 4)] and planted(0x4001, 4) == [] and planted(0x4001, 5) == [(0x4001, 0x4001, 5)]
    assert planted(0x8000, 5) == [(0x8000, 0x8000, 5)] and planted(0x8001, 5) == [] and planted(0x8001, 6) == [(0x8001, 0x8001, 6)]
    assert planted(0x20000, 6) == [(0x20000, 0x20000, 6)] and planted(0x20001, 7) == [] and planted(0x20001, 8) == [(0x20001, 0x20001, 8)]
    assert planted(0x80000, 7) == [] and planted(0x80000, 8) == [(0x80000, 0x80000, 8)] and planted(0x80000, 40) == [(0x80000, 0x80000, 40)]
    assert planted(0x80001, 8) == [] and planted(0x80001, 40) == []


# ---------------------------------------------------------------------------------------------- the built library
def test_library_exports_the_six_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def test_prototypes_agree_in_header_abi_and_shim():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), SB._c_param_types(m.group(3))) for m in re.finditer(r"\b(int|size_t)\s+(alz_bitenc_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(protos) == sorted(NAMES) and sorted(A.BITENC_PROTOTYPES) == sorted(NAMES)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"const alz_settings\*", C.c_void_p), (r"alz_result\*", C.c_void_p),
                (r"struct alz_file_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p), (r"size_t\*", C.POINTER(C.c_size_t)), (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    cs_of = SB.C_TO_CS + [(r"struct alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        ret, params = protos[name]
        assert A.BITENC_PROTOTYPES[name] == [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in params], name
        assert getattr(lib, name).argtypes == A.BITENC_PROTOTYPES[name]
        assert (getattr(lib, name).restype is C.c_size_t) == (ret == "size_t") == (name in A.BITENC_RESTYPES), name
        m = re.search(r"\[DllImport\(Lib(?:, ExactSpelling = true)?\)\]\s+internal static extern (\w+) %s\(([^)]*)\)" % name, native)
        assert m and m.group(1) == ("UIntPtr" if ret == "size_t" else "int"), name
        cs = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        assert len(cs) == len(params), name
        for ct, cst in zip(params, cs):
            assert cst == next(w for rx, w in cs_of if re.fullmatch(rx, ct)), (name, ct, cst)
    from auroralib.compression_amd.batch import Context
    from auroralib.compression_amd import formats as F
    for m in ("bitenc_encode_batch", "bitenc_encode_batch_device", "bitenc_file_compress_batch"):
        assert callable(getattr(Context, m))
    for cls in (F.CRILAYLA, F.ALLZ):
        assert callable(cls.Encode) and callable(cls.EncodeMany) and cls not in F.ALL_FORMATS
        assert "Encode" in F.BITLZ_NO_ENCODER


def test_pinned_constants_are_unchanged_and_the_internal_ids_stay_internal():
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert re.search(r"ALZ_BITLZ_CRILAYLA = 0, ALZ_BITLZ_ALLZ = 1, ALZ_BITLZ_COUNT = 2", text)
    assert "ALZ_FMT_CRILAYLA" not in text and "ALZ_FMT_ALLZ" not in text and "ALZ_ENCFMT" not in text
    bits = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "alz_bitlz.h")).read()
    assert re.search(r"ALZ_ENCFMT_CRILAYLA = ALZ_FMT_COUNT \+ 1, ALZ_ENCFMT_ALLZ = ALZ_FMT_COUNT \+ 2, ALZ_ENCFMT_COUNT = ALZ_FMT_COUNT \+ 3", bits)


def test_bounds_and_host_side_refusals_without_a_device():
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    assert lib.alz_bitenc_bound(A.BITLZ_CRILAYLA, 0) == 0 and lib.alz_bitenc_bound(A.BITLZ_CRILAYLA, 8) == 9 and lib.alz_bitenc_bound(A.BITLZ_CRILAYLA, 9) == 11
    assert lib.alz_bitenc_bound(A.BITLZ_ALLZ, 0) >= 1 and lib.alz_bitenc_bound(2, 100) == 0
    assert lib.alz_bitenc_file_bound(A.BITLZ_CRILAYLA, 0xFF) == 0 and lib.alz_bitenc_file_bound(A.BITLZ_CRILAYLA, 0x100) == 16 + 0x100
    assert lib.alz_bitenc_file_bound(A.BITLZ_ALLZ, 0) == 12 + lib.alz_bitenc_bound(A.BITLZ_ALLZ, 0)
    # the restated bodies stay within the bounds on what expands most: random bytes, and literals only
    rng = random.Random(2)
    for n in (1, 2, 3, 7, 64, 1000):
        data = bytes(rng.randrange(256) for _ in range(n))
        assert len(E.cri_compress_headerless(data, 0)) <= lib.alz_bitenc_bound(A.BITLZ_CRILAYLA, n)
        for triple in ((0, 0, 0), (24, 24, 24), (0, 10, 1)):
            assert len(E.allz_compress_headerless(data, 0, *triple)) <= lib.alz_bitenc_bound(A.BITLZ_ALLZ, n), (n, triple)


def test_kernel_hash_family():
    """the kernels stand in alz_encode_bits.h, a header alz_encode.hip includes and a file of the family "encode": every csrc header and kernel file is listed in
    a family, so none falls into both hashes, and the committed counters belong to these sources"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    csrc = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
    listed = set(sum(KH.FAMILIES.values(), []))
    assert not [f for f in os.listdir(csrc) if f.endswith((".h", ".hip")) and f not in listed]
    assert "alz_encode_bits.h" in KH.FAMILIES["encode"] and '#include "alz_encode_bits.h"' in open(os.path.join(csrc, "alz_encode.hip")).read()
    hip = open(os.path.join(csrc, "alz_encode_bits.h")).read()
    assert all(k in hip for k in ("enc_bits_cri_kernel", "enc_bits_allz_kernel", "enc_bits_reverse_kernel"))
    for name in KH.FILES:
        assert KH.recorded(name).get("encode") == KH.kernel_hash("encode") and KH.recorded(name).get("decode") == KH.kernel_hash("decode"), name
    assert "alz_bitenc_file.cpp" in open(os.path.join(csrc, "build.sh")).read()


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    notes = MC._kernel_notes(tmp_path)
    k = {n: v for n, v in notes.items() if "enc_bits_" in n}
    assert len(k) == 3 and all(sum(w in n for n in k) == 1 for w in ("enc_bits_reverse_kernel", "enc_bits_cri_kernel", "enc_bits_allz_kernel")), sorted(k)
    # the two lone-lane bodies are instances of enc_emit_kernel (the internal formats 26 and 27)
    emit = {n: v for n, v in notes.items() if re.search(r"enc_emit_kernelILi(%d|%d)E" % (A.FMT_COUNT + 1, A.FMT_COUNT + 2), n)}
    assert len(emit) == 2, sorted(emit)
    for n, v in {**k, **emit}.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
    assert sum("alz_bitlz" in n for n in notes) == 2
