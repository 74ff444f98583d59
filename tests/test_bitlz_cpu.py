"""No GPU: CRILAYLA and ALLZ (alz_bitlz_*, alz_crilayla_*, alz_allz_*).  The pure-Python restatement (tests/bitlz_ref.py) against the
hand-assembled known answers, the test-only stream makers against that restatement, the int32 rules of ReadALFlag, and the built library:
exported symbols, prototypes at every layer, the pinned ABI constants, the host-side header code of the two file layers, kernel resource
notes, the kernel-hash family, the refusal of Compress."""
import ctypes as C
import importlib.util
import json
import os
import random
import re
import subprocess
import sys

import pytest

import bitlz_ref as R
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_bitlz_decode_batch", "alz_bitlz_decode_batch_device", "alz_crilayla_is_match", "alz_crilayla_decompressed_size",
         "alz_crilayla_decompress", "alz_allz_is_match", "alz_allz_decompressed_size", "alz_allz_decompress")
TRIPLES = ((0, 10, 1), (0, 0, 0), (2, 8, 3), (5, 14, 2))


def kats():
    return json.load(open(os.path.join(GOLDEN, "bitlz_kat.json")))["cases"]


def ref_matches_kat(c, got):
    """got = (bytes, status, dst_len, src_used) of the restatement for a body case"""
    out, status, dst_len, src_used = got
    return (status == c["status"] and (c["dst_len"] is None or dst_len == c["dst_len"]) and src_used == c["src_used"]
            and (c["out"] is None or out == bytes.fromhex(c["out"])) and len(out) == dst_len)


def cri_random_tokens(rng, nbytes):
    toks, produced = [], 0
    while produced < nbytes:
        if produced < 3 or rng.random() < 0.4:
            toks.append(("lit", rng.randrange(256))); produced += 1
        else:
            d = min(rng.choice([3, 4, 5, 8, 17, 64, 100, 1000, 4096, 8193, 8194]), produced)
            L = rng.choice([3, 4, 5, 6, 12, 13, 43, 44, 100, 298, 299, 553, 554, 900])
            toks.append(("match", d, L)); produced += L
    return toks


def allz_random_tokens(rng, nbytes):
    toks = [("run", bytes(rng.randrange(256) for _ in range(rng.randrange(1, 9))))]
    produced = len(toks[0][1])
    while produced < nbytes:
        d = min(rng.choice([1, 2, 3, 7, 16, 64, 100, 1000, 5000, 70000]), produced)
        L = rng.choice([3, 4, 5, 8, 17, 64, 300, 2000])
        toks.append(("match", d, L)); produced += L
        if rng.random() < 0.6:
            n = rng.choice([1, 2, 3, 7, 16, 17, 100, 600])
            toks.append(("run", bytes(rng.randrange(256) for _ in range(n)))); produced += n
    return toks


def wrap_cases():
    """(name, src, decom_len, cap, params): ReadALFlag where the C# int arithmetic shows -- unary prefixes that take `bits` to 30, 31, 32 and 33
    (start bits 1: `ones` = bits - 1), as run length, distance and match length"""
    cases = []

    def stream(build):
        w = R.AllzWriter()
        build(w)
        return w.bytes()

    def run_src(bits, value):       # a run whose length field has `bits` bits (len_bits 1), eight raw bytes, then its match: distance 1, length 3
        return stream(lambda w: (w.bit(0), w.rawflag(bits - 1, value, bits), w.raw(b"abcdefgh"), w.rawflag(0, 0, 10), w.rawflag(0, 0, 0)))

    def len_src(bits, value):       # "xy", a match at distance 2 whose length field has `bits` bits (copy_bits 1), then the run "Z"
        return stream(lambda w: (w.bit(0), w.rawflag(0, 1, 1), w.raw(b"xy"), w.rawflag(0, 1, 10), w.rawflag(bits - 1, value, bits), w.bit(0), w.rawflag(0, 0, 1), w.raw(b"Z")))

    def dist_src(bits, value):      # "xy", a match of length 3 whose distance field has `bits` bits (dist_bits 1), then the run "Z"
        return stream(lambda w: (w.bit(0), w.rawflag(0, 1, 1), w.raw(b"xy"), w.rawflag(bits - 1, value, bits), w.rawflag(0, 1, 0), w.bit(0), w.rawflag(0, 0, 1), w.raw(b"Z")))

    for bits in (30, 31, 32, 33):
        for value in (0, 1, 2, 5, (1 << (bits - 1)) | 3):
            cases.append(("run field of %d bits, value %#x" % (bits, value), run_src(bits, value), 40, 40, (0, 10, 1)))
            cases.append(("run field of %d bits, value %#x, dst_cap 6" % (bits, value), run_src(bits, value), 40, 6, (0, 10, 1)))
            cases.append(("length field of %d bits, value %#x" % (bits, value), len_src(bits, value), 50, 50, (1, 10, 1)))
            cases.append(("distance field of %d bits, value %#x" % (bits, value), dist_src(bits, value), 50, 50, (0, 1, 1)))
    # 33 bits: the addend is ((1 << 0) - 1) << 1 = 0 and bit 32 of the field lands on bit 0 -- streams that end where decom_len says
    cases.append(("run field of 33 bits, 2^32 + 6 reads 7", run_src(33, (1 << 32) | 6), 11, 11, (0, 10, 1)))
    cases.append(("length field of 33 bits, 4 reads 4", len_src(33, 4), 10, 10, (1, 10, 1)))
    cases.append(("distance field of 33 bits, 2^32 reads 1", dist_src(33, 1 << 32), 6, 6, (0, 1, 1)))
    return cases


# ---------------------------------------------------------------------------------------------- the restatement
def test_kat_file_is_what_its_generator_writes():
    spec = importlib.util.spec_from_file_location("make_bitlz_kats_t", os.path.join(GOLDEN, "make_bitlz_kats.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.CASES == kats()
    names = " | ".join(c["name"] for c in m.CASES)
    for need in ("crilayla: literals, a match", "dst_cap inside the last match", "input ends inside the last token", "distance beyond the bytes produced",
                 "crilayla: empty input", "as a file", "allz: runs, matches", "decom_len inside the last match", "dst_cap below decom_len",
                 "decom_len beyond what the input holds", "allz: cut to 0 bytes", "allz: cut to 10 bytes", "a match as the first token", "the body as a file"):
        assert need in names, need
    src = open(os.path.join(GOLDEN, "make_bitlz_kats.py")).read()
    assert "bitlz_ref" not in src.split('"""')[2] and "import ctypes" not in src          # the generator calls no decoder


@pytest.mark.parametrize("k", range(len(kats())), ids=lambda k: kats()[k]["name"].replace(" ", "_"))
def test_ref_against_kat(k):
    c = kats()[k]
    src = bytes.fromhex(c["src"])
    if c["file"] and c["kind"] == "crilayla":
        assert R.cri_file_decode(src) == ("ok", c["status"], bytes.fromhex(c["out"]), c["src_used"])
    elif c["file"]:
        got = R.allz_decode(src[12:], int.from_bytes(src[8:12], "little"), None, src[5], src[6], src[7])
        assert src[:4] == b"ALLZ" and (got[0], got[1], got[2], got[3] + 12) == (bytes.fromhex(c["out"]), c["status"], c["dst_len"], c["src_used"])
    elif c["kind"] == "crilayla":
        assert ref_matches_kat(c, R.cri_decode(src, c["cap"]))
    else:
        assert ref_matches_kat(c, R.allz_decode(src, c["decom_len"], c["cap"], *c["params"]))


def test_issue_values():
    """the figures the feature request quotes"""
    by = {c["name"]: c for c in kats()}
    c = by["crilayla: literals, a match, an overlapping match"]
    assert c["src"] == "107e0048440070889020" and bytes.fromhex(c["out"]) == b"ACDBACDBACDBACDBACBACBA" and (c["status"], c["dst_len"], c["src_used"]) == (R.OK, 23, 10)
    c = by["crilayla: dst_cap inside the last match"]
    assert bytes.fromhex(c["out"]) == b"CDBACDBACDBACDBACBACBA" and (c["status"], c["dst_len"]) == (R.CAPACITY, 22)
    c = by["crilayla: input ends inside the last token"]
    assert c["src"] == "7e0048440070889020" and bytes.fromhex(c["out"]) == b"DBACBACBA" and (c["status"], c["src_used"]) == (R.TRUNC, 9)
    c = by["crilayla: distance beyond the bytes produced"]
    assert c["src"] == "0000a09020" and bytes.fromhex(c["out"]) == b"BA" and (c["status"], c["src_used"]) == (R.BAD, 5)
    c = by["crilayla: the first body as a file"]
    assert c["src"].startswith("4352494c41594c41170000000a000000") and (c["dst_len"], c["src_used"]) == (279, 282)
    c = by["allz: runs, matches, an overlapping match"]
    assert c["src"] == "82414243000d003044c011" and bytes.fromhex(c["out"]) == b"ABCABCABBBBDBBBDBBBDBBBDBB" and (c["status"], c["src_used"]) == (R.OK, 11)
    assert (by["allz: decom_len inside the last match"]["status"], by["allz: decom_len inside the last match"]["dst_len"]) == (R.MISMATCH, 25)
    assert (by["allz: dst_cap below decom_len"]["status"], by["allz: dst_cap below decom_len"]["dst_len"]) == (R.CAPACITY, 25)
    c = by["allz: decom_len beyond what the input holds"]
    assert (c["status"], c["dst_len"], c["src_used"]) == (R.TRUNC, 26, 11)
    c = by["allz: a match as the first token"]
    assert c["src"] == "0100" and (c["status"], c["dst_len"], c["src_used"]) == (R.BAD, 0, 2)
    assert by["allz: the body as a file"]["src"].startswith("414c4c5a00000a011a000000")


def test_makers_reproduce_the_hand_assembled_streams():
    toks = [("lit", 0x41), ("lit", 0x42), ("lit", 0x43), ("match", 3, 5), ("lit", 0x44), ("match", 4, 14)]
    assert R.cri_assemble(toks).hex() == "107e0048440070889020" and R.cri_expected(toks)[::-1] == b"ACDBACDBACDBACDBACBACBA"
    assert R.cri_assemble(toks, pad=1).hex() == "1f7e0048440070889020"
    toks = [("run", b"ABC"), ("match", 3, 5), ("match", 1, 3), ("run", b"D"), ("match", 4, 14)]
    assert R.allz_assemble(toks).hex() == "82414243000d003044c011" and R.allz_expected(toks) == b"ABCABCABBBBDBBBDBBBDBBBDBB"


def test_crilayla_maker_round_trips_through_the_restatement():
    rng = random.Random(1)
    fields = set()
    for t in range(250):
        toks = cri_random_tokens(rng, rng.randrange(1, 2500))
        fields |= {len(R.cri_token_bits(k)) for k in toks if k[0] == "match"}
        body, plain = R.cri_assemble(toks, pad=t & 1), R.cri_expected(toks)
        assert R.cri_decode(body, len(plain) + (t % 3)) == (plain[::-1], R.OK, len(plain), len(body)), t
    assert fields >= {16, 19, 24, 32, 40}                                         # one to five length fields


def test_allz_maker_round_trips_through_the_restatement():
    rng = random.Random(2)
    for t in range(200):
        params = TRIPLES[t % 4]
        toks = allz_random_tokens(rng, rng.randrange(1, 4000))
        body, plain = R.allz_assemble(toks, *params), R.allz_expected(toks)
        assert R.allz_decode(body, len(plain), len(plain) + (t % 3), *params) == (plain, R.OK, len(plain), len(body)), (t, params)


def test_every_cut_is_truncated_and_every_capacity_clips():
    rng = random.Random(7)
    toks = cri_random_tokens(rng, 150)
    body, plain = R.cri_assemble(toks), R.cri_expected(toks)
    for cut in range(1, len(body) + 1):                                           # bytes dropped at the FRONT are the ones read last
        out, status, n, used = R.cri_decode(body[cut:], 4096)
        assert status in (R.TRUNC, R.OK) and used == len(body) - cut and out == plain[:n][::-1], cut
    assert sum(R.cri_decode(body[cut:], 4096)[1] == R.TRUNC for cut in range(1, len(body))) > len(body) // 2
    for cap in range(len(plain)):
        assert R.cri_decode(body, cap) == (plain[:cap][::-1], R.CAPACITY, cap, None), cap
    for params in TRIPLES:
        toks = allz_random_tokens(rng, 120) + [("match", 2, 5)]
        body, plain = R.allz_assemble(toks, *params), R.allz_expected(toks)
        n = len(plain)
        for cut in range(len(body)):
            out, status, k, used = R.allz_decode(body[:cut], n, n, *params)
            assert (status, used) == (R.TRUNC, cut) and out == plain[:k], (params, cut)
        for cap in range(n):
            assert R.allz_decode(body, n, cap, *params) == (plain[:cap], R.CAPACITY, cap, None), (params, cap)
        for decom in range(n):
            out, status, k, used = R.allz_decode(body, decom, n, *params)
            assert out == plain[:decom] and k == decom and status in (R.OK, R.MISMATCH), (params, decom)
            assert (status == R.OK) == (decom in {len(R.allz_expected(toks[:j])) for j in range(len(toks) + 1)}), (params, decom)
        assert R.allz_decode(body, n + 1, n + 1, *params)[1:] == (R.TRUNC, n, len(body))


def test_read_al_flag_follows_the_int32_rules():
    def one(bits, value, raw=bytes(range(1, 41)), tail=False):
        """a run whose length field has `bits` bits (start bits 1), `raw` behind it, then (tail) a match of distance 1 and length 3"""
        w = R.AllzWriter()
        w.bit(0); w.rawflag(bits - 1, value, bits); w.raw(raw)
        if tail:
            w.rawflag(0, 0, 10); w.rawflag(0, 0, 0)
        return R.allz_decode(w.bytes(), 30, 30, 0, 10, 1)

    # bits 30: + ((1 << 29) - 1) << 1 = 0x3FFFFFFE; the run is far longer than the span: clipped, OUTPUT_SIZE_MISMATCH with what fits
    assert one(30, 0) == (bytes(range(1, 31)), R.MISMATCH, 30, None)
    # bits 31: + 0x7FFFFFFE; + 1 = int.MaxValue, still positive
    assert one(31, 0) == (bytes(range(1, 31)), R.MISMATCH, 30, None)
    assert one(31, 0, raw=b"abc") == (b"abc", R.TRUNC, 3, 8 + 3)                    # 1 + 30 + 1 + 31 bits = 8 flag bytes; fewer bytes than the clipped run needs
    # bits 32: ((1 << 31) - 1) << 1 wraps to 0xFFFFFFFE = -2.  value 0 -> run -1: BAD_TOKEN behind the field (1 + 31 + 1 + 32 bits = 9 flag bytes)
    assert one(32, 0) == (b"", R.BAD, 0, 9)
    # ... value 1 -> run 0: copies nothing, and the match that has to follow finds nothing produced: BAD_TOKEN behind ITS fields
    assert one(32, 1, raw=b"", tail=True) == (b"", R.BAD, 0, 10)
    # ... value 3 -> run 2, then the match
    assert one(32, 3, raw=b"pq", tail=True)[:3] == (b"pqqqq", R.TRUNC, 5)
    # bits 33: 1 << (32 mod 32) = 1: the addend is 0, and bit 32 of the field lands on bit 0 (`1 << i` takes i mod 32)
    assert one(33, 4, raw=b"12345", tail=True)[0] == b"12345555" and one(33, 1 << 32, raw=b"12", tail=True)[0] == b"12222" and one(33, (1 << 32) | 1, raw=b"12", tail=True)[0] == b"12222"
    # a distance that wraps to <= 0 with a positive length is BAD_TOKEN; with a length <= 0 it is nothing at all
    statuses = {}
    for name, src, decom, cap, params in wrap_cases():
        got = R.allz_decode(src, decom, cap, *params)
        statuses.setdefault(got[1], []).append(name)
        assert len(got[0]) == got[2] <= min(decom, cap), name
    assert set(statuses) == {R.OK, R.TRUNC, R.MISMATCH, R.CAPACITY, R.BAD}, {k: len(v) for k, v in statuses.items()}
    assert len(statuses[R.OK]) == 3 and any("run field of 32 bits, value 0x0" == n for n in statuses[R.BAD]) and any(n.startswith("distance field of 32 bits") for n in statuses[R.BAD])
    assert R.i32(0x7FFFFFFF + 1) == -(1 << 31) and R.i32(0xFFFFFFFE + 1) == -1


# ---------------------------------------------------------------------------------------------- the built library
def test_library_exports_the_eight_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def _header_protos():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    return {m.group(1): SB._c_param_types(m.group(2)) for m in re.finditer(r"\bint\s+(alz_(?:bitlz|crilayla|allz)_\w+)\s*\(([^)]*)\)\s*;", text)}


def test_prototypes_agree_in_header_abi_and_shim():
    protos = _header_protos()
    assert sorted(protos) == sorted(NAMES)
    assert sorted(A.BITLZ_PROTOTYPES) == sorted(NAMES)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"alz_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p),
                (r"uint32_t\*", C.POINTER(C.c_uint32)), (r"int32_t\*", C.POINTER(C.c_int32)), (r"size_t\*", C.POINTER(C.c_size_t)),
                (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    for name in NAMES:
        want = [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in protos[name]]
        assert A.BITLZ_PROTOTYPES[name] == want, name
        m = re.search(r"\[DllImport\(Lib\)\]\s+internal static extern int %s\(([^)]*)\)" % name, native)
        assert m, name
        cs = [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        assert len(cs) == len(protos[name]), name
        for ct, cst in zip(protos[name], cs):
            assert cst == next(w for rx, w in SB.C_TO_CS if re.fullmatch(rx, ct)), (name, ct, cst)
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == A.BITLZ_PROTOTYPES[name]
    from auroralib.compression_amd.batch import Context
    for m in ("bitlz_decode_batch", "bitlz_decode_batch_device"):
        assert callable(getattr(Context, m))


def test_pinned_abi_constants_are_unchanged():
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text)
    assert re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert (A.ABI_VERSION, A.FMT_COUNT, A.C_COUNT) == (2, 25, 46)
    assert re.search(r"ALZ_BITLZ_CRILAYLA = 0, ALZ_BITLZ_ALLZ = 1, ALZ_BITLZ_COUNT = 2", text)
    assert (A.BITLZ_CRILAYLA, A.BITLZ_ALLZ, A.BITLZ_COUNT) == (0, 1, 2)
    assert "ALZ_FMT_CRILAYLA" not in text and "ALZ_FMT_ALLZ" not in text
    assert A.allz_aux0() == 0 | 10 << 8 | 1 << 16 and A.allz_aux0(7, 20, 9) == 7 | 20 << 8 | 9 << 16
    m = re.search(r"#define ALZ_ALLZ_AUX0\(copy_bits, dist_bits, len_bits\)\s+\(\(copy_bits\) \| \(dist_bits\) << 8 \| \(len_bits\) << 16\)", text)
    assert m


def test_is_match_and_decompressed_size_on_the_library():
    from auroralib.compression_amd import _lib
    from auroralib.compression_amd import formats as F
    lib = _lib.load()
    size = C.c_uint32(0)
    # CRILAYLA: Length > 0x10 and the magic; size + 0x100 in 32 bits
    f = R.cri_file(bytes(4), 1234, bytes(0x100))
    assert lib.alz_crilayla_is_match(f[:17], 17) == 1 and lib.alz_crilayla_is_match(f[:16], 16) == 0
    assert lib.alz_crilayla_is_match(b"CRILAYLB" + f[8:], len(f)) == 0 and lib.alz_crilayla_is_match(b"crilayla" + f[8:], len(f)) == 0
    assert lib.alz_crilayla_decompressed_size(f, len(f), C.byref(size)) == 0 and size.value == 1234 + 0x100
    assert lib.alz_crilayla_decompressed_size(f[:12], 12, C.byref(size)) == 0 and size.value == 1234 + 0x100
    assert lib.alz_crilayla_decompressed_size(f[:11], 11, C.byref(size)) == A.E_FORMAT
    assert lib.alz_crilayla_decompressed_size(b"CRILAYLB" + f[8:], len(f), C.byref(size)) == A.E_FORMAT
    w = R.cri_file(b"", 0xFFFFFF80, b"")
    assert lib.alz_crilayla_decompressed_size(w, len(w), C.byref(size)) == 0 and size.value == 0x80          # the uint sum wraps
    assert lib.alz_crilayla_decompressed_size(f, len(f), None) == A.E_INVALID
    cl = F.CRILAYLA()
    assert cl.IsMatch(f) and not cl.IsMatch(f[:16]) and cl.GetDecompressedSize(f) == 1234 + 0x100
    with pytest.raises(F.InvalidIdentifierException):
        cl.GetDecompressedSize(b"XRILAYLA" + f[8:])
    # ALLZ: Position + 0x10 < Length and the magic; the u32 at 8
    g = R.allz_file(bytes(8), 4321, 3, 9, 2)
    assert len(g) == 20 and g[4:8] == bytes([0, 3, 9, 2])
    assert lib.alz_allz_is_match(g[:17], 17) == 1 and lib.alz_allz_is_match(g[:16], 16) == 0
    assert lib.alz_allz_is_match(b"ALLY" + g[4:], 20) == 0 and lib.alz_allz_is_match(b"allz" + g[4:], 20) == 0
    assert lib.alz_allz_decompressed_size(g, 20, C.byref(size)) == 0 and size.value == 4321
    assert lib.alz_allz_decompressed_size(g[:12], 12, C.byref(size)) == 0 and size.value == 4321
    assert lib.alz_allz_decompressed_size(g[:11], 11, C.byref(size)) == A.E_FORMAT
    assert lib.alz_allz_decompressed_size(b"ALLY" + g[4:], 20, C.byref(size)) == A.E_FORMAT
    az = F.ALLZ()
    assert az.IsMatch(g) and not az.IsMatch(g[:16]) and az.GetDecompressedSize(g) == 4321
    with pytest.raises(F.InvalidIdentifierException):
        az.GetDecompressedSize(b"XLLZ" + g[4:])


def test_python_classes_refuse_compress_and_stay_outside_all_formats():
    from auroralib.compression_amd import formats as F
    for cls in (F.CRILAYLA, F.ALLZ):
        with pytest.raises(NotImplementedError) as e:
            cls().Compress(b"abc")
        assert cls.__name__ in str(e.value) and "no oracle body to hold bit-identity against" in str(e.value)
        assert cls not in F.ALL_FORMATS
        for m in ("IsMatch", "GetDecompressedSize", "Decompress", "Compress"):
            assert callable(getattr(cls, m))
    assert F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20] and F.APLib not in F.ALL_FORMATS
    az = F.ALLZ()
    assert (az.LzCopyBits, az.LzDistanceBits, az.LzLengthBits) == (0, 10, 1)


def test_kernel_hash_family():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["bitlz"] == ["alz_bitlz.hip", "alz_bitlz.h"]
    assert KH.FAMILIES["aplib"] == ["alz_aplib.hip", "alz_aplib.h"] and KH.FAMILIES["rlh"] == ["alz_rlh.hip", "alz_rlh.h"]
    for fam in KH.FAMILIES:
        files = KH.family_files(fam)
        assert ("alz_bitlz.hip" in files) == (fam == "bitlz") and ("alz_bitlz.h" in files) == (fam == "bitlz"), fam
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_bitlz.hip" in build and "alz_bitlz_file.cpp" in build


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_bitlz" in n}
    assert len(k) == 2 and sum("alz_bitlz_crilayla_kernel" in n for n in k) == 1 and sum("alz_bitlz_allz_kernel" in n for n in k) == 1, sorted(k)
    for n, v in k.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
    assert not any("alz_aplib" in n or "alz_measure_" in n for n in k)
