"""No GPU: RLHudson (alz_rlhudson_*).  The pure-Python restatement (tests/rlhudson_ref.py) against hand-assembled known answers, the managed
encoder's defect, and the built library: declarations and exported symbols, ctypes prototypes, the encode bound, the argument checks that
need no context, the constants this family must leave alone, and the resource notes of the new kernels."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_measure_cpu as MC
import test_shim_binding as SB
import rlhudson_ref as W
from auroralib.compression_amd import _abi as A
from cases import prose_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ("alz_rlhudson_decode_batch", "alz_rlhudson_decode_batch_device", "alz_rlhudson_encode_batch", "alz_rlhudson_encode_batch_device")
KERNELS = ("alz_rlh_hudson_decode_exact_kernel", "alz_rlh_hudson_decode_kernel", "alz_rlh_hudson_encode_kernel")


def nonrepeating(n):
    """bytes without two equal neighbours: nothing for the run finder"""
    return bytes((7 * i + (i >> 8)) & 0xFF for i in range(n))


# ---------------------------------------------------------------------------------------------- the restatement
# (name, stream, decom_len, dst_cap, bytes, status, dst_len, src_used) -- assembled by hand from RLHudson.cs:54-81; src_used None: unspecified
KATS = [
    ("run", "0561", 5, 5, b"aaaaa", W.OK, 5, 2),
    ("literals", "8378797a", 3, 3, b"xyz", W.OK, 3, 4),
    ("run of 0 writes nothing", "00090162", 1, 1, b"b", W.OK, 1, 4),
    ("0 literals write nothing", "808164", 1, 1, b"d", W.OK, 1, 3),
    ("run of 127", "7f63", 127, 127, b"c" * 127, W.OK, 127, 2),
    ("ends at a control byte", "0301", 10, 10, b"\1\1\1", W.INPUT_TRUNCATED, 3, 2),
    ("ends at a run byte", "030105", 10, 10, b"\1\1\1", W.INPUT_TRUNCATED, 3, 3),
    ("ends inside a literal run", "0301846162", 10, 10, b"\1\1\1", W.INPUT_TRUNCATED, 3, 5),
    ("only empty elements, then the end", "80800000", 1, 1, b"", W.INPUT_TRUNCATED, 0, 4),
    ("overshoot", "03010902", 5, 64, b"\1\1\1" + b"\2" * 9, W.OUTPUT_SIZE_MISMATCH, 12, 4),
    ("dst_cap inside a run", "03010902", 12, 7, b"\1\1\1\2\2\2\2", W.OUTPUT_CAPACITY, 7, None),
    ("dst_cap inside a literal run", "03018461626364", 7, 5, b"\1\1\1ab", W.OUTPUT_CAPACITY, 5, None),
    ("dst_cap met by the overshooting token", "03010902", 5, 7, b"\1\1\1\2\2\2\2", W.OUTPUT_SIZE_MISMATCH, 7, 4),
    ("decom_len 0", "0301", 0, 0, b"", W.OK, 0, 0),
]


@pytest.mark.parametrize("k", range(len(KATS)), ids=lambda k: KATS[k][0].replace(" ", "_"))
def test_ref_against_known_answer(k):
    name, src, size, cap, out, status, dst_len, used = KATS[k]
    got = W.rlhudson_decode(bytes.fromhex(src), size, cap)
    assert got[:3] == (out, status, dst_len), name
    if used is None:
        assert status == W.OUTPUT_CAPACITY and got[3] is None
    else:
        assert got[3] == used, name


def test_every_control_byte():
    """each of the 256 control bytes in front of 127 bytes: what it writes and how much input it takes"""
    body = bytes(range(1, 128))
    for c in range(256):
        n = c & 0x7F
        out, st, ln, used = W.rlhudson_decode(bytes([c]) + body, n, 200)
        if n == 0:
            assert (out, st, ln, used) == (b"", W.OK, 0, 0)                    # the loop never runs: RLHudson.cs:60
            out, st, ln, used = W.rlhudson_decode(bytes([c]) + body + b"\x01\x55", 1, 200)
            # `00 01`: an empty run, then control 02 = a run of 2 x 03 (an overshoot of 1); `80`: empty literals, then control 01 = a run of 1 x 02
            assert (out, st, used) == ((b"\3\3", W.OUTPUT_SIZE_MISMATCH, 4) if c == 0 else (b"\2", W.OK, 3))
        elif c < 0x80:
            assert (out, st, ln, used) == (bytes([1]) * n, W.OK, n, 2), c
        else:
            assert (out, st, ln, used) == (body[:n], W.OK, n, 1 + n), c


def test_encoder_tokens_and_defect():
    """RLHudson.cs:83-102 over RleMatchFinder(3, 0x7F); `duration = source.Length - offset` (RleMatchFinder.cs:43) makes literal runs of 128 / 129
    bytes, whose control bytes come out as 0x80 / 0x81: those streams do not decode back."""
    E = W.rlhudson_encode
    assert E(b"") == b"" and E(b"a") == b"\x81a" and E(b"ab") == b"\x82ab" and E(b"abc") == b"\x83abc" and E(b"aaa") == b"\x03a"
    assert E(b"aa") == b"\x82aa" and E(b"q" * 127) == b"\x7fq" and E(b"q" * 128) == b"\x7fq\x81q" and E(b"q" * 130) == b"\x7fq\x03q"
    assert E(b"ab" + b"c" * 5 + b"de") == b"\x82ab\x05c\x82de"
    assert E(nonrepeating(127)) == b"\xff" + nonrepeating(127)
    assert E(nonrepeating(128)) == b"\x80" + nonrepeating(128)                 # the defect: 128 | 0x80 -> 0x80
    assert E(nonrepeating(129)) == b"\x81" + nonrepeating(129)                 # ... 129 | 0x80 -> 0x81
    assert E(nonrepeating(130)) == b"\xff" + nonrepeating(127) + b"\x83" + nonrepeating(130)[127:]
    for n, ok in ((126, True), (127, True), (128, False), (129, False), (130, True), (254, True), (255, False), (256, False), (257, True)):
        data = nonrepeating(n)
        out, st, ln, _ = W.rlhudson_decode(E(data), n, n + 300)
        assert ((st == W.OK and out == data) is ok) and W.rlhudson_has_defect(data) is (not ok), (n, st, ln)
    for data in (b"", b"a", b"ab", b"abc", b"aaa", b"aab", b"a" * 127, b"a" * 128, b"a" * 130, b"ab" + b"c" * 300 + b"de", prose_like(5000, 2), bytes(3000)):
        comp = E(data)
        assert len(comp) <= W.rlhudson_encode_bound(len(data))
        assert W.rlhudson_decode(comp, len(data), len(data)) == (data, W.OK, len(data), len(comp)), data[:8]


# ---------------------------------------------------------------------------------------------- the library, without a GPU
def _lib():
    from auroralib.compression_amd._lib import load
    return load()


def test_header_and_python_declare_the_entry_points():
    protos, types = SB._header_prototypes(), MC._header_types()
    for name in BATCH:
        assert protos.get(name) == 8, name
        c, py = types[name], A.RLHUDSON_PROTOTYPES[name]
        assert len(c) == len(py) == 8
        for ct, pt in zip(c, py):
            assert pt is (C.c_void_p if ct.endswith("*") else {"uint32_t": C.c_uint32, "size_t": C.c_size_t}[ct]), (name, ct, pt)
        assert py == A.RLH_PROTOTYPES["alz_rlh_decode_batch"]                  # the parameter list of its alz_rlh_* twin
    assert protos.get("alz_rlhudson_encode_bound") == 1 and A.RLHUDSON_PROTOTYPES["alz_rlhudson_encode_bound"] == [C.c_size_t]
    from auroralib.compression_amd.batch import Context
    for m in ("rlhudson_decode_batch", "rlhudson_encode_batch", "rlhudson_decode_batch_device", "rlhudson_encode_batch_device"):
        assert callable(getattr(Context, m))


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    lib = _lib()
    for name in BATCH + ("alz_rlhudson_encode_bound",):
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(lib, name).argtypes == A.RLHUDSON_PROTOTYPES[name]
    assert lib.alz_rlhudson_encode_bound.restype is C.c_size_t
    for n in (0, 1, 3, 127, 129, 1 << 20, (1 << 32) + 5):
        assert lib.alz_rlhudson_encode_bound(n) == W.rlhudson_encode_bound(n)


def test_the_family_leaves_the_pinned_constants_alone():
    """RLHudson is no fourth alz_rlh_format and no alz_format: it has entry points of its own"""
    hdr = open(SB.HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", hdr)
    for text, val in (("ALZ_RLH_COUNT", 3), ("ALZ_C_COUNT ", 46), ("ALZ_FMT_COUNT ", 25)):
        assert re.search(re.escape(text) + r"\s*=\s*%d\b" % val, hdr), text
    assert (A.ABI_VERSION, A.RLH_COUNT, A.C_COUNT, A.FMT_COUNT) == (2, 3, 46, 25)
    assert _lib().alz_abi_version() == 2
    from auroralib.compression_amd import formats as F
    assert F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20]
    assert not re.search(r"HUDSON", re.search(r"typedef enum alz_rlh_format \{[^}]*\}", hdr).group(0), re.I)


def test_argument_checks_need_no_context():
    lib = _lib()
    s = (A.Stream * 1)(A.Stream(0, 0, 2, 5, 5, 0, 0, 0))
    res = (A.Result * 1)()
    src, dst = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    for name in BATCH:
        assert getattr(lib, name)(None, 1, src, 64, s, dst, 64, res) == A.E_INVALID, name      # a NULL context
        assert getattr(lib, name)(None, 0, None, 0, None, None, 0, None) == A.E_INVALID, name


def test_hudson_kernels_exist_and_use_no_scratch(tmp_path):
    notes = MC._kernel_notes(tmp_path)
    for k in KERNELS:
        hit = [n for n in notes if re.search(r"\d%s[A-Z]" % k, n) or n == k]
        assert len(hit) == 1, (k, sorted(n for n in notes if "alz_rlh" in n))
        v = notes[hit[0]]
        print("%s: %d VGPRs, %d B LDS" % (k, v["vgpr_count"], v["group_segment_fixed_size"]))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    # one template over a grammar trait: the production kernel has RLE30's LDS footprint
    lds = {n: v["group_segment_fixed_size"] for n, v in notes.items() if "decode_kernel" in n and ("rle30" in n or "hudson" in n)}
    assert len(lds) == 2 and len(set(lds.values())) == 1, lds
