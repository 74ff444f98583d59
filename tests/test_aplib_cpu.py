"""No GPU: aPLib (alz_aplib_*).  The pure-Python restatement (tests/aplib_ref.py) against the hand-assembled known answers, the two test-only
stream makers against that restatement, and the built library: exported symbols, prototypes at every layer, the pinned ABI constants, the
host-side header code of the file layer, kernel resource notes, the kernel-hash family, the refusal of Compress."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import random
import re
import subprocess
import sys

import pytest

import aplib_ref as R
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A
from cases import prose_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_aplib_decode_batch", "alz_aplib_decode_batch_device", "alz_aplib_measure_batch", "alz_aplib_measure_batch_device",
         "alz_aplib_is_match", "alz_aplib_decompressed_size", "alz_aplib_decompress")


def kats():
    return json.load(open(os.path.join(GOLDEN, "aplib_kat.json")))["cases"]


def kat_matches(c, out):
    if "out" in c:
        return out == bytes.fromhex(c["out"])
    return hashlib.sha256(out).hexdigest() == c["out_sha256"] and out[:64].hex() == c["out_head"] and out[-64:].hex() == c["out_tail"]


def word_soup(rng, n):
    """a few short words and runs of small bytes: matches at many distances, one-byte tokens, repeats"""
    words = [bytes(rng.randrange(256) for _ in range(rng.randrange(1, 9))) for _ in range(20)]
    return b"".join(rng.choice(words) if rng.random() < 0.8 else bytes(rng.randrange(3)) for _ in range(n)) or b"x"


# ---------------------------------------------------------------------------------------------- the restatement
def test_kat_file_is_what_its_generator_writes():
    spec = importlib.util.spec_from_file_location("make_aplib_kats_t", os.path.join(GOLDEN, "make_aplib_kats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.CASES == kats()
    names = " | ".join(c["name"] for c in m.CASES)
    for need in ("every token kind", "dst_cap inside a match", "dst_cap 0", "behind the end marker", "ends at a distance byte", "inside a length gamma",
                 "empty input", "one byte", "repeat as the first token", "gamma wraps", "= the window (2 MiB)", "the window + 1"):
        assert need in names, need
    src = open(os.path.join(GOLDEN, "make_aplib_kats.py")).read()
    assert "aplib_ref" not in src.split('"""')[2] and "import ctypes" not in src          # the generator calls no decoder


@pytest.mark.parametrize("k", range(len(kats())), ids=lambda k: kats()[k]["name"].replace(" ", "_"))
def test_ref_against_kat(k):
    c = kats()[k]
    out, status, dst_len, src_used = R.decode(bytes.fromhex(c["src"]), c["cap"])
    assert (status, dst_len) == (c["status"], c["dst_len"]) and len(out) == dst_len
    assert kat_matches(c, out)
    if c["src_used"] is not None:
        assert src_used == c["src_used"]
    else:
        assert status == R.CAPACITY and src_used is None


def test_issue_values():
    """the figures the feature request quotes"""
    by = {c["name"]: c for c in kats()}
    c = by["every token kind"]
    assert c["src"] == "4172 42c8 0743 6807 e890 4e18 00".replace(" ", "") and bytes.fromhex(c["out"]) == b"ABAABACBACBAACBACBAAC" + bytes(5)
    assert (c["status"], c["dst_len"], c["src_used"]) == (R.OK, 26, 13)
    assert (by["distance = the window (2 MiB)"]["status"], by["distance = the window (2 MiB)"]["dst_len"]) == (R.OK, 2097261)
    bad = by["distance = the window + 1"]
    assert (bad["status"], bad["dst_len"], bad["src_used"], len(bad["src"]) // 2) == (R.BAD, 2097253, 85, 87)
    assert bytes.fromhex(by["gamma wraps at 32 bits"]["out"]) == bytes([1, 0, 0, 0, 0])


def test_assemble_reproduces_the_hand_assembled_stream():
    toks = [("lit", 0x42), ("one", 2), ("short", 3, 3), ("lit", 0x43), ("rep", 5), ("match", 7, 9), ("match", 0x90, 4), ("one", 0), ("end",)]
    assert R.assemble(0x41, toks).hex() == kats()[0]["src"]
    assert R.assemble(1, [("gmatch", (1 << 33) | 5, 0x10, 4), ("end",)]).hex() == [c for c in kats() if c["name"].startswith("gamma wraps")][0]["src"]


def test_greedy_and_assemble_round_trip():
    rng = random.Random(1)
    kinds = set()
    for t in range(30):
        data = word_soup(rng, rng.randrange(1, 3000))
        first, toks = R.greedy_tokens(data)
        kinds |= {k[0] for k in toks}
        comp = R.assemble(first, toks)
        assert comp == R.greedy(data)
        out, status, dst_len, src_used = R.decode(comp, len(data) + 8)
        assert (out, status, dst_len, src_used) == (data, R.OK, len(data), len(comp)), t
    assert kinds == {"lit", "one", "short", "match", "rep", "end"}
    data = prose_like(20000, 5)
    comp = R.greedy(data)
    assert len(comp) < len(data) * 3 // 4
    assert R.decode(comp, len(data)) == (data, R.OK, len(data), len(comp))


def test_every_prefix_is_truncated_and_every_cap_is_capacity():
    comp = R.greedy(word_soup(random.Random(7), 60))
    full = R.decode(comp, 1 << 20)
    assert full[1] == R.OK
    for cut in range(len(comp)):
        out, status, dst_len, src_used = R.decode(comp[:cut], 1 << 20)
        assert status == R.TRUNC and src_used == cut and out == full[0][:dst_len], cut
    for cap in range(full[2]):
        out, status, dst_len, src_used = R.decode(comp, cap)
        assert (status, dst_len, src_used) == (R.CAPACITY, cap, None) and out == full[0][:cap], cap
    assert R.decode(comp, full[2]) == full


def test_wrapped_arithmetic():
    # (g - 3) << 8 negative as an int: refused behind the length gamma
    s = R.assemble(0x55, [("gmatch", 0x00800003, 0x01, 2), ("end",)])
    assert R.decode(s, 100) == (b"\x55", R.BAD, 1, len(s) - 1)                     # (just behind the length gamma: the end marker's byte is not read)
    # length <= 0 after the wrap copies nothing; lastOffset and lwm are updated (the next gamma 2 is NOT a repeat: bias 2 -> distance 0x00 << 8 | low)
    s = R.assemble(0x55, [("lit", 0x66), ("gmatch", 3, 0x01, 0x80000000), ("gmatch", 2, 0x02, 2), ("end",)])
    assert R.decode(s, 100)[:3] == (b"\x55\x66\x55\x66\x55\x66", R.OK, 6)
    # the input ends inside the length gamma of a bad-distance token: truncated wins
    s = R.assemble(0x55, [("gmatch", 0x00800003, 0x01, 1 << 20)])
    assert R.decode(s[:-1], 100)[1:] == (R.TRUNC, 1, len(s) - 1)


# ---------------------------------------------------------------------------------------------- the built library
def test_library_exports_the_seven_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _header_protos():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(1): SB._c_param_types(m.group(2)) for m in re.finditer(r"\bint\s+(alz_aplib_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_prototypes_agree_in_header_abi_and_shim():
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert sorted(A.APLIB_PROTOTYPES) == sorted(NAMES)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"int32_t\*", C.POINTER(C.c_int32)), (r"size_t\*", C.POINTER(C.c_size_t)),
                (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    for name in NAMES:
        want = [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in protos[name]]
        assert A.APLIB_PROTOTYPES[name] == want, name
        m = re.search(r"\[DllImport\(Lib\)\]\s+internal static extern int %s\(([^)]*)\)" % name, native)
        assert m, name
        cs = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        assert len(cs) == len(protos[name]), name
        for ct, cst in zip(protos[name], cs):
            assert cst == next(w for rx, w in SB.C_TO_CS if re.fullmatch(rx, ct)), (name, ct, cst)
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == A.APLIB_PROTOTYPES[name]
    from auroralib.compression_amd.batch import Context
    for m in ("aplib_decode_batch", "aplib_decode_batch_device", "aplib_measure_batch", "aplib_measure_batch_device"):
        assert callable(getattr(Context, m))


def test_pinned_abi_constants_are_unchanged():
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text)
    assert re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert (A.ABI_VERSION, A.FMT_COUNT) == (2, 25)
    assert "ALZ_FMT_APLIB" not in text and "THERE IS NO ENCODER" in text


def _file(header_size=24, comp=b"", size=0, pad=b""):
    return b"AP32" + header_size.to_bytes(4, "little") + len(comp).to_bytes(4, "little") + bytes(4) + size.to_bytes(4, "little") + bytes(4) + pad + comp


def test_is_match_and_decompressed_size_on_the_library():
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    f = _file(24, bytes(8), 1234)
    assert len(f) == 32
    assert lib.alz_aplib_is_match(f[:17], 17) == 1 and lib.alz_aplib_is_match(f[:16], 16) == 0                 # Position + 0x10 < Length
    assert lib.alz_aplib_is_match(b"AP33" + f[4:], 32) == 0 and lib.alz_aplib_is_match(b"ap32" + f[4:], 32) == 0
    for hs in (0, 20, 23, 25, 32, 0x18000000):
        assert lib.alz_aplib_is_match(_file(hs, bytes(8), 1), 32) == 0, hs                                     # ReadUInt32() == 24
    size = C.c_uint32(0)
    assert lib.alz_aplib_decompressed_size(f, 32, C.byref(size)) == 0 and size.value == 1234
    assert lib.alz_aplib_decompressed_size(f[:20], 20, C.byref(size)) == 0 and size.value == 1234
    assert lib.alz_aplib_decompressed_size(f[:19], 19, C.byref(size)) == A.E_FORMAT
    assert lib.alz_aplib_decompressed_size(b"AP33" + f[4:], 32, C.byref(size)) == A.E_FORMAT
    assert lib.alz_aplib_decompressed_size(_file(32, b"", 77, bytes(8)), 32, C.byref(size)) == 0 and size.value == 77   # (any header size)
    from auroralib.compression_amd import formats as F
    ap = F.APLib()
    assert ap.IsMatch(f) and not ap.IsMatch(f[:16]) and ap.GetDecompressedSize(f) == 1234
    with pytest.raises(F.InvalidIdentifierException):
        ap.GetDecompressedSize(b"XP32" + f[4:])


def test_python_class_refuses_compress_and_stays_outside_all_formats():
    from auroralib.compression_amd import formats as F
    with pytest.raises(NotImplementedError) as e:
        F.APLib().Compress(b"abc")
    assert "LzChainMatchFinder" in str(e.value) and "oracle" in str(e.value)
    assert F.APLib not in F.ALL_FORMATS and F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20]
    for m in ("IsMatch", "GetDecompressedSize", "Decompress", "Compress"):
        assert callable(getattr(F.APLib, m))


def test_kernel_hash_family():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["aplib"] == ["alz_aplib.hip", "alz_aplib.h"]
    for fam in KH.FAMILIES:
        files = KH.family_files(fam)
        assert ("alz_aplib.hip" in files) == (fam == "aplib") and ("alz_aplib.h" in files) == (fam == "aplib"), fam
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_aplib.hip" in build


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_aplib" in n}
    assert len(k) == 3 and any("alz_aplib_measure_kernel" in n for n in k), sorted(k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
    assert not any("alz_measure_exact_kernel" in n or "alz_measure_bulk_kernel" in n for n in k)
