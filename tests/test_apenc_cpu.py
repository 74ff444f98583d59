"""No GPU: aPLib written (alz_apenc_*).  The oracle has no aPLib, so the yardstick of the GPU tests is a Python restatement (tests/apenc_ref.py:
aPLib.CompressHeaderless and Compress, over the finder of tests/chain_finder_ref.py, which tests/test_bitenc_cpu.py pins to the oracle).  Here that
restatement is checked: it round-trips through the restated reader, its byte placement agrees with an independent assembler at every flag phase of
both hand-over rules, the finder obeys the seven property sets at their edges, and the `lengthDelta < 2` branch of the managed code is dead.  Then
the built library: exported symbols, prototypes at every layer, bounds, the pinned constants, kernel resource notes, the kernel-hash family.
CPU time of the module: about 30 s, 20 of them the 2 MiB input of tests/golden/apenc_far.json."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import pytest

import apenc_ref as E
import aplib_ref as R
import chain_finder_ref as CF
import test_bitenc_cpu as BC
import test_gpu_apenc as G               # (the builders of the planted inputs: shared with the GPU tests, which compare bytes on them)
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "auroralz.h")
NAMES = ("alz_apenc_bound", "alz_apenc_encode_batch", "alz_apenc_encode_batch_device", "alz_apenc_file_bound", "alz_apenc_file_compress",
         "alz_apenc_file_compress_batch")
SETS = ((0x1000, E.INT_MAX, 3), (0x80, 3, 2), (0x4000, E.INT_MAX, 4), (0x10000, E.INT_MAX, 5), (0x40000, E.INT_MAX, 6), (0x100000, E.INT_MAX, 7), (0x200000, E.INT_MAX, 8))


# ---------------------------------------------------------------------------------------------- the restatement
def test_restatement_round_trips_through_the_restated_reader(test_bmp):
    inputs = [d for d in BC._inputs(test_bmp) if d] + [test_bmp[:1], test_bmp[:100], test_bmp[:4000]]
    seen = {}
    for data in inputs:
        for q in (0, 1, 4, 8, 10, 12, 15):
            for strategy in (0, 1):
                body = E.compress_headerless(data, q, strategy, seen)
                out, status, n, used = R.decode(body, len(data))
                assert (status, n, out, used) == (R.OK, len(data), data, len(body)), (len(data), q, strategy)
                assert len(body) <= E.bound(len(data))
    assert seen.get("dead", 0) == 0 and all(seen.get(k, 0) > 0 for k in ("lit", "one", "short", "rep", "match", "match_biased")), seen
    with pytest.raises(IndexError):
        E.compress_headerless(b"", 8)                                        # source[srcPtr++] of an empty span


def test_file_form_has_the_six_header_words(test_bmp):
    data = test_bmp[:3000]
    f = E.compress(data, 8)
    body = E.compress_headerless(data, 8)
    assert f[:4] == b"AP32" and [int.from_bytes(f[4 + 4 * k:8 + 4 * k], "little") for k in range(5)] == [24, len(body), 0, len(data), 0] and f[24:] == body


def tokens_of(data, match_list):
    """the token list aplib_ref.assemble wants, from the format's rules alone (what a position IS; where its bits and bytes go is the assembler's own business)"""
    toks, sp, last_end, last_d = [], 1, None, 0
    for offset, d, ln in match_list:
        for p in range(sp, offset):
            b = data[p]
            off = 0 if b == 0 else next((i for i in range(1, min(16, p + 1)) if data[p - i] == b), -1)
            toks.append(("one", off) if off >= 0 else ("lit", b))
        if ln == 0:
            break
        if last_end != offset and last_d == d:
            toks.append(("rep", ln))
        elif ln <= 3 and d <= 127:
            toks.append(("short", d, ln))
        else:
            toks.append(("match", d, ln))
        sp, last_end, last_d = offset + ln, offset + ln, d
    return data[0], toks + [("end",)]


def test_emit_against_the_independent_assembler_by_hand():
    """every token kind, the pair bias and a repeat, written out by hand"""
    data = b"QabcdeXabcdeYabZ\x00cdecdeW"
    #        0123456789012345   6789012 3
    ml = [(7, 6, 5), (13, 6, 2), (17, 8, 3), (20, 3, 3), (len(data), 0, 0)]
    toks = [("lit", ord(c)) for c in "abcdeX"] + [("match", 6, 5),          # no match before it: the pair bias (high = 0 + 3)
            ("lit", ord("Y")), ("rep", 2),                                   # the last distance again, behind a literal: a repeat
            ("lit", ord("Z")), ("one", 0),                                   # a zero byte
            ("short", 8, 3), ("short", 3, 3),                                # three bytes at distance 8, three at distance 3 right behind them
            ("lit", ord("W")), ("end",)]
    stats = {}
    got = E.emit(data, ml, stats)
    assert got == R.assemble(ord("Q"), toks) and R.decode(got, len(data)) == (data, R.OK, len(data), len(got))
    assert stats == {"lit": 9, "match_biased": 1, "rep": 1, "one": 1, "short": 2}
    assert tokens_of(data, ml) == (ord("Q"), toks)
    # a normal block right behind a match (lwm: no bias), and one whose distance has a high part
    seg = bytes(range(1, 41))
    far = bytes(range(60, 200)) * 3
    data = seg + far + seg[:6] + seg[10:16] + far[:300]
    ml = [(140 + 40, 140, 280), (460, 460, 6), (466, 456, 6), (472, 432, 300), (len(data), 0, 0)]
    first, toks = tokens_of(data, ml)
    assert [t for t in toks if t[0] in ("match", "rep", "short")] == [("match", 140, 280), ("match", 460, 6), ("match", 456, 6), ("match", 432, 300)]
    stats = {}
    assert E.emit(data, ml, stats) == R.assemble(first, toks) and stats["match"] == 3 and stats["match_biased"] == 1


def test_emit_at_every_flag_phase_of_both_hand_over_rules():
    """k literals in front shift every later token by k bits: a literal, a short block, the end marker (the byte, then one more bit) and a normal block's low byte
    (the byte, then FlushIfNecessary) are handed over at each of the eight phases, the flag byte that fills exactly on the gamma in front of a low byte included"""
    rule_a, rule_b = set(), set()
    for k in range(8):
        lead = bytes(range(200, 200 + k))
        seg = b"ABCDEFGH"
        data = b"\x01" + lead + seg + b"ij" + seg[:6] + b"k" + b"ij" + b"lmnopqrs"
        o1 = 1 + k + 8 + 2
        ml = [(o1, 10, 6), (o1 + 7, 9, 2), (len(data), 0, 0)]
        trace = []
        got = E.emit(data, ml, None, trace)
        first, toks = tokens_of(data, ml)
        assert [t for t in toks if t[0] in ("match", "short")] == [("match", 10, 6), ("short", 9, 2)]
        assert got == R.assemble(first, toks), k
        assert R.decode(got, len(data))[:3] == (data, R.OK, len(data))
        for kind, pos, bits, d, ln in trace:
            if kind == "lit":
                rule_a.add(("lit", bits % 8))
            elif kind in ("short", "end"):
                rule_a.add((kind, (bits + 2) % 8))
            elif kind == "match_biased":
                rule_b.add((bits + 2 + 2 * (((d >> 8) + 3).bit_length() - 1)) % 8)      # `10`, gamma(high): the bits written when the low byte enters Buffer
    assert rule_b == set(range(8)), rule_b                                    # (phase 0: the flag byte is full, the low byte goes out at once)
    for kind in ("lit", "short", "end"):
        assert {p for kd, p in rule_a if kd == kind} == set(range(8)), (kind, rule_a)


def test_the_seven_sets_in_the_restated_finder():
    """ScoreMatch takes the first set that admits a candidate.  Sets 0..4 on the planted inputs the GPU tests encode: at each set's last distance its minimum length
    is taken and one byte less is not, one byte further the minimum is not taken and the next set's is.  (Two and three bytes only come from the min-length
    table, from quality 10 on: the chain hashes four.)  Sets 5 and 6 -- 0x100000 and 0x200000 -- are in the golden file, below."""
    taken = {(t[3], t[4]): t[0] for t in G.traced(G.edge_input(), 10) if t[0] in G.MATCH_KINDS}
    assert taken[(0x7F, 2)] == "short" and taken[(0x7F, 3)] == "short" and taken[(0x80, 2)] == "match_biased" and taken[(0x80, 3)] == "match_biased"   # set 1: (0x80, 3, 2)
    data, plants = G.wide_input()
    taken = {(t[3], t[4]): t[0] for t in G.traced(data, 10) if t[0] in G.MATCH_KINDS}
    for mx, mn in G.SET_EDGES:
        assert (mx, mn) in taken and (mx, mn - 1) not in taken and (mx + 1, mn) not in taken and (mx + 1, mn + 1) in taken, (hex(mx), mn)
    # set 1's far edge: two bytes at 0x81 belong to no set, three to set 0
    near = G.planted_input([(0x81, 2, False), (0x80, 2, False), (0x81, 3, False)], 600, 12, gap=150)
    taken = {(t[3], t[4]) for t in G.traced(near, 10) if t[0] in G.MATCH_KINDS}
    assert (0x81, 2) not in taken and (0x80, 2) in taken and (0x81, 3) in taken
    # every match the finder returned on these inputs obeys the first set that admits its distance ... and at quality 8 nothing shorter than four bytes is found
    for d, ln in taken:
        assert any(d <= mx and mn <= ln <= ml for mx, ml, mn in SETS), (d, ln)
    assert not [t for t in G.traced(near, 8) if t[0] in G.MATCH_KINDS]
    assert min(t[4] for t in G.traced(G.edge_input(), 8) if t[0] in G.MATCH_KINDS) == 4


def test_golden_far_inputs_are_what_the_restatement_gives():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_apenc_kats as K
    committed = json.load(open(os.path.join(ROOT, "tests", "golden", "apenc_far.json")))
    assert sorted(committed) == sorted(K.CASES)
    for name, case in K.CASES.items():
        assert committed[name] == json.loads(json.dumps(K.answer(case))), name
    far = committed["far"]["far_matches"]
    assert far == [[0x100000, 7], [0x100001, 8], [0x1FFFFF, 8], [0x200000, 8]]     # six bytes at 0x100000, seven at 0x100001 and 0x200000, anything at 0x200001: left alone
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "apenc_far.json")) < 4096


def test_the_length_delta_branch_is_dead():
    """aPLib.cs:256-259 `if (lengthDelta < 2) continue;` would leave srcPtr where it is and lose the match.  For every distance at a set's edge or a LengthDelta
    edge and every length ScoreMatch can return for it, in every state of (lwm, lastOffset): where the normal form is reached, L - LengthDelta(D) >= 2."""
    f = CF.ChainFinder(E.APLIB_LZ, 10)
    edges = sorted({1, 2, 0x7F, 0x80, 0x81, 0x4FF, 0x500, 0x501, 0x7CFF, 0x7D00, 0x7D01} | {mx + k for mx, _, _ in SETS for k in (-1, 0, 1)})
    reached = {"rep": 0, "short": 0, "normal": 0}
    for d in edges:
        for found in range(2, 20):
            score, ln = f._score(found, d)
            if score < 0 or ln < f.min_len:
                continue                                                     # (no set admits it: FindNextBestMatch never returns it)
            for lwm in (False, True):
                for last in (d, d + 1):
                    if not lwm and last == d and ln >= 2:
                        reached["rep"] += 1
                    elif ln <= 3 and d <= 127:
                        reached["short"] += 1
                    else:
                        reached["normal"] += 1
                        assert ln - R.length_delta(d) >= 2, (hex(d), ln)
    assert all(reached.values()), reached
    assert f._score(2, 0x80) == (0, 2) and R.length_delta(0x80) == 0 and f._score(2, 0x81) == (-1, 0)      # the tightest case: two bytes at 0x80
    assert f._score(3, 0x500)[1] - R.length_delta(0x500) == 2 and f._score(5, 0x7D00)[1] - R.length_delta(0x7D00) == 3


# ---------------------------------------------------------------------------------------------- the built library
def test_library_exports_the_six_functions():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name


def test_prototypes_agree_in_header_abi_and_shim():
    text = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    protos = {m.group(2): (m.group(1), SB._c_param_types(m.group(3))) for m in re.finditer(r"\b(int|size_t)\s+(alz_apenc_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(protos) == sorted(NAMES) and sorted(A.APENC_PROTOTYPES) == sorted(NAMES)
    ctype_of = [(r"alz_ctx\*", C.c_void_p), (r"const alz_stream\*", C.c_void_p), (r"const alz_settings\*", C.c_void_p), (r"alz_result\*", C.c_void_p),
                (r"struct alz_file_result\*", C.c_void_p), (r"(?:const )?uint8_t\*", C.c_void_p), (r"size_t\*", C.POINTER(C.c_size_t)), (r"uint32_t", C.c_uint32), (r"size_t", C.c_size_t)]
    cs_of = SB.C_TO_CS + [(r"struct alz_file_result\*", "AlzFileResult*")]
    native = open(os.path.join(SB.SHIM, "Native.cs")).read()
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        ret, params = protos[name]
        assert A.APENC_PROTOTYPES[name] == [next(t for rx, t in ctype_of if re.fullmatch(rx, ct)) for ct in params], name
        assert getattr(lib, name).argtypes == A.APENC_PROTOTYPES[name]
        assert (getattr(lib, name).restype is C.c_size_t) == (ret == "size_t") == (name in A.APENC_RESTYPES), name
        m = re.search(r"\[DllImport\(Lib(?:, ExactSpelling = true)?\)\]\s+internal static extern (\w+) %s\(([^)]*)\)" % name, native)
        assert m and m.group(1) == ("UIntPtr" if ret == "size_t" else "int"), name
        cs = [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        assert len(cs) == len(params), name
        for ct, cst in zip(params, cs):
            assert cst == next(w for rx, w in cs_of if re.fullmatch(rx, ct)), (name, ct, cst)
    from auroralib.compression_amd.batch import Context
    from auroralib.compression_amd import formats as F
    for m in ("apenc_encode_batch", "apenc_encode_batch_device", "apenc_file_compress_batch"):
        assert callable(getattr(Context, m))
    assert callable(F.APLib.Encode) and callable(F.APLib.EncodeMany) and F.APLib not in F.ALL_FORMATS
    with pytest.raises(NotImplementedError) as e:
        F.APLib().Compress(b"abc")
    assert "LzChainMatchFinder" in str(e.value) and "oracle" in str(e.value) and "Encode" in str(e.value)


def test_pinned_constants_are_unchanged_and_the_internal_id_stays_internal():
    text = open(HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", text) and re.search(r"\bALZ_FMT_COUNT\s*=\s*25\b", text) and re.search(r"\bALZ_C_COUNT\s*=\s*46\b", text)
    assert "ALZ_FMT_APLIB" not in text and "ALZ_ENCFMT" not in text and "THERE IS NO ENCODER" in text and "alz_apenc_" in text
    assert "NOT BUILT: aPLib" not in text
    bits = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "alz_bitlz.h")).read()
    assert re.search(r"ALZ_ENCFMT_CRILAYLA = ALZ_FMT_COUNT \+ 1, ALZ_ENCFMT_ALLZ = ALZ_FMT_COUNT \+ 2, ALZ_ENCFMT_COUNT = ALZ_FMT_COUNT \+ 3", bits)
    assert re.search(r"^enum \{ ALZ_ENCFMT_APLIB = ALZ_FMT_COUNT \+ 3, ALZ_ENCFMT_END = ALZ_FMT_COUNT \+ 4 \};$", bits, flags=re.M)
    assert len(re.findall(r"\b(?:int|size_t)\s+alz_aplib_\w+\s*\(", text)) == 7 and len(re.findall(r"\b(?:int|size_t)\s+alz_bitenc_\w+\s*\(", text)) == 6


def test_bounds_without_a_device():
    from auroralib.compression_amd import _lib
    lib = _lib.load()
    assert [lib.alz_apenc_bound(n) for n in (0, 1, 8, 64)] == [0, 3, 11, 74] == [E.bound(n) for n in (0, 1, 8, 64)]
    assert [lib.alz_apenc_file_bound(n) for n in (0, 1, 64)] == [24, 27, 98]
    assert lib.alz_apenc_bound(0x40000000) == E.bound(0x40000000)
    rng = random.Random(2)
    for n in (1, 2, 3, 7, 8, 9, 64, 200):                                     # literals only (no byte equals one of the fifteen before it, none is zero): the bound itself
        assert len(E.compress_headerless(G.ramp(n), 0)) == lib.alz_apenc_bound(n), n
    for n in (1, 2, 3, 7, 64, 1000, 5000):
        for q in (0, 10):
            assert len(E.compress_headerless(bytes(rng.randrange(256) for _ in range(n)), q)) <= lib.alz_apenc_bound(n), (n, q)


def test_kernel_hash_family_and_build_list():
    """the kernels stand in alz_encode_bits.h, a header alz_encode.hip includes and a file of the family "encode": every csrc header and kernel file is listed in a
    family, the families are the ones tools/kernel_hash.py lists, and the committed counters belong to these sources"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    csrc = os.path.join(ROOT, "auroralib", "compression_amd", "csrc")
    listed = set(sum(KH.FAMILIES.values(), []))
    assert not [f for f in os.listdir(csrc) if f.endswith((".h", ".hip")) and f not in listed]
    assert sorted(KH.FAMILIES) == ["aplib", "bitlz", "checksum", "decode", "encode", "filebatch", "framing", "inflate", "measure", "rlh", "xxh32", "zfile"]
    hip, bits = open(os.path.join(csrc, "alz_encode.hip")).read(), open(os.path.join(csrc, "alz_encode_bits.h")).read()
    assert "alz_encode_bits.h" in KH.FAMILIES["encode"] and '#include "alz_encode_bits.h"' in hip
    assert "enc_gamma_ap_kernel" in bits and "aplib_emit_lone" in bits and "ALZ_ENCFMT_APLIB" in hip
    for name in KH.FILES:
        assert KH.recorded(name).get("encode") == KH.kernel_hash("encode") and KH.recorded(name).get("decode") == KH.kernel_hash("decode"), name
    assert "alz_apenc_file.cpp" in open(os.path.join(csrc, "build.sh")).read()


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    notes = MC._kernel_notes(tmp_path)
    k = {n: v for n, v in notes.items() if "enc_gamma_" in n}
    assert len(k) == 1 and "enc_gamma_ap_kernel" in next(iter(k)), sorted(k)
    emit = {n: v for n, v in notes.items() if re.search(r"enc_emit_kernelILi%dE" % (A.FMT_COUNT + 3), n)}     # the lone-lane body: one more instance of enc_emit_kernel
    assert len(emit) == 1, sorted(emit)
    for n, v in {**k, **emit}.items():
        print(n, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)
    assert next(iter(k.values()))["group_segment_fixed_size"] == 4 * (96 + 64 + 64)                            # ALZ_GAMMA_WIN_DWORDS and the two per-lane arrays
    assert sum("alz_aplib" in n for n in notes) == 3 and sum("enc_bits_" in n for n in notes) == 3 and sum("alz_bitlz" in n for n in notes) == 2
