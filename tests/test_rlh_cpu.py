"""No GPU: the RLE30 / HUF20 family (alz_rlh_*).  The pure-Python restatement (tests/rlh_ref.py) against the hand-assembled known answers, the
test-only HUF20 builder against that restatement, the managed RLE30 encoder's defect, and the built library: exported symbols, prototypes at
every layer, the host-side header code of containers 44 / 45, the refusals of the Huffman encoder, kernel resource notes, the kernel-hash family."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess

import numpy as np
import pytest

import rlh_ref as R
import test_measure_cpu as MC
import test_shim_binding as SB
from auroralib.compression_amd import _abi as A
from cases import prose_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("alz_rlh_decode_batch", "alz_rlh_decode_batch_device", "alz_rlh_encode_batch", "alz_rlh_encode_batch_device")


def kats():
    return json.load(open(os.path.join(GOLDEN, "rlh_kat.json")))["cases"]


def nonrepeating(n):
    """bytes without two equal neighbours: nothing for the run finder"""
    return bytes((7 * i + (i >> 8)) & 0xFF for i in range(n))


# ---------------------------------------------------------------------------------------------- the restatement
def test_kat_file_is_what_its_generator_writes(tmp_path):
    spec = importlib.util.spec_from_file_location("make_kats_rlh_t", os.path.join(GOLDEN, "make_kats_rlh.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.CASES == kats()
    names = " | ".join(c["name"] for c in m.CASES)
    for need in ("run of 3", "run of 130", "literal run of 1 ", "literal run of 128", "overshoot", "ends at a control byte", "ends at a run byte",
                 "ends inside a literal run", "decom_len 0", "three leaves", "little nibble", "big nibble", "spanning a word boundary",
                 "short tree read", "treeSize 0", "index beyond the tree", "above 0xF", "without header bytes"):
        assert need in names, need


@pytest.mark.parametrize("k", range(len(kats())), ids=lambda k: kats()[k]["name"].replace(" ", "_"))
def test_ref_against_kat(k):
    c = kats()[k]
    out, status, dst_len, src_used = R.decode(c["fmt"], bytes.fromhex(c["src"]), c["decom_len"], c["cap"], c["aux0"])
    assert (status, dst_len) == (c["status"], c["dst_len"])
    assert out == bytes.fromhex(c["out"])
    if c["src_used"] is not None:
        assert src_used == c["src_used"]
    else:
        assert status == R.OUTPUT_CAPACITY


def fib_data(nsym):
    """Fibonacci frequencies over `nsym` symbols: the deepest tree a Huffman code makes of that many bytes"""
    f = [1, 1]
    while len(f) < nsym:
        f.append(f[-1] + f[-2])
    rng = np.random.default_rng(nsym)
    data = np.concatenate([np.full(n, s, dtype=np.uint8) for s, n in enumerate(f)])
    rng.shuffle(data)
    return data.tobytes()


def huf_sets():
    """(name, data, bit depths): the data sets of the GPU test, checked here to build and to decode back under the restatement"""
    rng = np.random.default_rng(20)
    eight = np.repeat(np.arange(8, dtype=np.uint8), 1024)
    rng.shuffle(eight)
    nib = (eight[0::2] | (eight[1::2] << 4)).astype(np.uint8).tobytes()       # 4096 bytes: 8 nibble values x 1024, all codes 3 bits
    u = np.repeat(np.arange(256, dtype=np.uint8), 20)
    rng.shuffle(u)
    uniform = u.tobytes()                                                     # 5120 bytes, every value 20 times: 255 nodes, all codes 8 bits
    return [
        ("two_symbols", bytes(rng.choice([0x11, 0x22], 3000).astype(np.uint8)), (8,)),
        ("fixed3", nib, (4,)),
        ("uniform", uniform, (8, 4)),
        ("fib16", fib_data(16), (8,)),
        ("fib20", fib_data(20), (8,)),
        ("prose", prose_like(6000, 5), (8, 4)),
        ("one", b"\x5a", (8, 4)), ("two", b"\x5a\xa5", (8, 4)), ("odd1001", prose_like(1001, 6), (8, 4)),
    ]


def test_builder_streams_decode_back():
    assert len(fib_data(16)) == 2583 and len(fib_data(20)) == 17710
    for name, data, depths in huf_sets():
        for bits in depths:
            for big in ((False, True) if bits == 4 else (False,)):
                s = R.huf20_build(data, bits, big)
                assert s is not None, (name, bits)
                out, st, n, used = R.huf20_decode(s, len(data), len(data), bits, big)
                assert (st, n, used) == (R.OK, len(data), len(s)) and out == data, (name, bits, big)
    # the worst case is named: 8 nibble values, 1024 each -> every code has 3 bits (never self-synchronising)
    s = R.huf20_build(huf_sets()[1][1], 4)
    assert s[0] == 7 and len(s) == 2 + 14 + 4096 * 2 * 3 // 8
    s = R.huf20_build(huf_sets()[2][1], 8)
    assert s[0] == 255 and len(s) == 2 + 510 + 5120                           # uniform bytes: 255 nodes, all codes 8 bits


def test_builder_reports_what_the_layout_cannot_hold():
    """The None path of the builder, pinned on tree shapes handed to the label layout directly: a complete tree of depth 9 (511 nodes) fits
    neither the size byte nor, at its widest level, the 6-bit offsets; the same shape at depth 8 (255 nodes, what 256 equally frequent bytes
    give) is laid out and walks back to its leaves.  (No byte histogram was found that overflows an offset -- the Score order of
    BuildLabelTreeList keeps children close -- so the data sets of the GPU test all build.)"""
    def complete(d, sym=[0]):
        if d == 0:
            sym[0] += 1
            return R._Node(1, (sym[0] - 1) & 0xFF)
        return R._Node(1, None, complete(d - 1), complete(d - 1))
    assert R.huf20_label(complete(9)) is None
    hdr = R.huf20_label(complete(8))
    assert hdr is not None and hdr[0] == 255 and len(hdr) == 2 + 510
    body = bytes([0x00, 0xFF, 0x5A, 0x00])                                        # the word 0x005AFF00, little-endian: three 8-bit codes, their bits are the leaf numbers
    assert R.huf20_decode(bytes(hdr) + body, 3, 3, 8)[:3] == (bytes([0x00, 0x5A, 0xFF]), R.OK, 3)


def test_rle30_encoder_defect_at_129_and_256():
    """RleMatchFinder.cs:41-45: `duration = source.Length - offset` makes a literal run of 129 whose control byte wraps to 0x80."""
    for n, ok in ((128, True), (129, False), (130, True), (256, False)):
        data = nonrepeating(n)
        comp = R.rle30_encode(data)
        out, st, ln, _ = R.rle30_decode(comp, n, n + 200)
        assert ((st == R.OK and out == data) is ok), (n, st, ln)
    comp = R.rle30_encode(nonrepeating(129))
    assert comp[0] == 0x80 and len(comp) == 130                               # one token: control (129 - 1) & 0xFF, 129 literals
    comp = R.rle30_encode(nonrepeating(256))
    assert comp[0] == 126 and comp[128] == 0x80 and len(comp) == 258          # 127 literals, then a run of 129 literals
    for data in (b"", b"a", b"ab", b"abc", b"aaa", b"aab", b"a" * 127, b"a" * 128, b"a" * 130, b"ab" + b"c" * 300 + b"de", prose_like(5000, 2), bytes(3000)):
        comp = R.rle30_encode(data)
        out, st, ln, used = R.rle30_decode(comp, len(data), len(data))
        assert (st, out, used) == (R.OK, data, len(comp)), data[:8]


# ---------------------------------------------------------------------------------------------- the library, without a GPU
def _lib():
    from auroralib.compression_amd._lib import load
    return load()


def test_header_python_and_shim_declare_the_entry_points():
    protos, types = SB._header_prototypes(), MC._header_types()
    imports = SB._dllimports()
    for name in NAMES:
        assert protos.get(name) == 8 and imports.get(name) == 8, name
        c, py = types[name], A.RLH_PROTOTYPES[name]
        assert len(c) == len(py) == 8
        for ct, pt in zip(c, py):
            assert pt is (C.c_void_p if ct.endswith("*") else {"uint32_t": C.c_uint32, "size_t": C.c_size_t}[ct]), (name, ct, pt)
    hdr = open(SB.HDR).read()
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", hdr)
    for text, val in (("ALZ_RLH_RLE30", A.RLH_RLE30), ("ALZ_RLH_HUF20_4", A.RLH_HUF20_4), ("ALZ_RLH_HUF20_8", A.RLH_HUF20_8), ("ALZ_RLH_COUNT", A.RLH_COUNT),
                      ("ALZ_C_RLE30 ", A.C_RLE30), ("ALZ_C_HUF20 ", A.C_HUF20), ("ALZ_C_COUNT ", A.C_COUNT), ("ALZ_FMT_COUNT ", 25)):
        assert re.search(re.escape(text) + r"\s*=\s*%d\b" % val, hdr), text
    for text, val in (("ALZ_LZ77_HUF20_4", 0x24), ("ALZ_LZ77_HUF20_8", 0x28), ("ALZ_LZ77_RLE30", 0x30), ("ALZ_LEVEL5_HUFFMAN4", 2), ("ALZ_LEVEL5_HUFFMAN8", 3), ("ALZ_LEVEL5_RLE", 4)):
        assert int(re.search(r"#define %s\s+(\w+?)u\b" % text, hdr).group(1), 0) == val, text
    assert (A.C_RLE30, A.C_HUF20, A.C_COUNT, A.FMT_COUNT) == (44, 45, 46, 25)


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
    lib = _lib()
    for name in NAMES:
        assert getattr(lib, name).argtypes == A.RLH_PROTOTYPES[name]


def _is_match(container, data):
    return _lib().alz_container_is_match(container, bytes(data), len(data))


def _size(container, data):
    v = C.c_uint32(0xDEAD)
    rc = _lib().alz_container_decompressed_size(container, None, bytes(data), len(data), C.byref(v))
    return rc, v.value


def test_container_headers_rle30_and_huf20():
    # RLE30.cs:33-34: Position + 6 <= Length, 0x30, (u24 != 0 || u32 != 0), then a non-zero byte (ReadUInt8: a read past the end throws)
    assert _is_match(A.C_RLE30, b"\x30\x05\x00\x00\x82\x41") == 1
    assert _is_match(A.C_RLE30, b"\x30\x05\x00\x00\x82") == 0                  # 5 bytes
    assert _is_match(A.C_RLE30, b"\x30\x05\x00\x00\x00\x41") == 0              # first body byte 0
    assert _is_match(A.C_RLE30, b"\x31\x05\x00\x00\x82\x41") == 0
    assert _is_match(A.C_RLE30, b"\x30\x00\x00\x00\x00\x00\x00\x01\x82") == 1  # u24 == 0 -> u32
    assert _is_match(A.C_RLE30, b"\x30\x00\x00\x00\x00\x00\x00\x00\x82") == 0  # both sizes 0
    assert _is_match(A.C_RLE30, b"\x30\x00\x00\x00\x00\x00\x00\x01") == 0      # nothing behind the u32
    # HUF20.cs:50-51: Position + 6 < Length, type 0x24 / 0x28, the sizes, ReadByte() != 0 (-1 at the end counts)
    for t in (0x24, 0x28):
        assert _is_match(A.C_HUF20, bytes([t, 5, 0, 0, 2, 0x80, 0x41])) == 1
        assert _is_match(A.C_HUF20, bytes([t, 5, 0, 0, 2, 0x80])) == 0         # 6 bytes: not more than 6
        assert _is_match(A.C_HUF20, bytes([t, 5, 0, 0, 0, 0x80, 0x41])) == 0
        assert _is_match(A.C_HUF20, bytes([t, 0, 0, 0, 9, 0, 0, 0])) == 1      # u32 form, the byte behind it missing: -1 != 0
        assert _is_match(A.C_HUF20, bytes([t, 0, 0, 0, 9, 0, 0, 0, 0])) == 0
        assert _is_match(A.C_HUF20, bytes([t, 0, 0, 0, 0, 0, 0, 0, 3])) == 0
    assert _is_match(A.C_HUF20, bytes([0x20, 5, 0, 0, 2, 0x80, 0x41])) == 0
    assert _is_match(A.C_HUF20, bytes([0x30, 5, 0, 0, 2, 0x80, 0x41])) == 0
    # RLE30.cs:40-50 / HUF20.cs:57-67
    assert _size(A.C_RLE30, b"\x30\x05\x04\x03") == (0, 0x030405)
    assert _size(A.C_RLE30, b"\x30\x00\x00\x00\x78\x56\x34\x12") == (0, 0x12345678)
    assert _size(A.C_RLE30, b"\x30\x00\x00\x00\x00\x00\x00\x00") == (0, 0)
    assert _size(A.C_RLE30, b"\x30\x00\x00\x00\x78\x56")[0] == A.E_FORMAT
    assert _size(A.C_RLE30, b"\x24\x05\x04\x03")[0] == A.E_FORMAT
    assert _size(A.C_HUF20, b"\x24\x05\x04\x03") == (0, 0x030405)
    assert _size(A.C_HUF20, b"\x28\x00\x00\x00\x78\x56\x34\x12") == (0, 0x12345678)
    assert _size(A.C_HUF20, b"\x30\x05\x04\x03")[0] == A.E_FORMAT
    for data in (R.gba_header(0x30, 77) + b"\x82A", R.gba_header(0x30, 0x1000000) + b"\x82A"):
        assert _is_match(A.C_RLE30, data) == 1 and _size(A.C_RLE30, data) == (0, 77 if len(data) == 6 else 0x1000000)


def test_huffman_compress_is_refused_everywhere():
    lib = _lib()
    lib.alz_container_compress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    dst, dl = C.create_string_buffer(256), C.c_size_t()

    def compress(container, variant, quality=8):
        o, st = A.ContainerOptions(), A.Settings(quality, 0, 0, 0)
        o.variant = variant
        return lib.alz_container_compress(None, container, C.byref(o), C.byref(st), b"abcdabcd", 8, dst, 256, C.byref(dl))
    assert compress(A.C_HUF20, 0) == A.E_UNSUPPORTED and compress(A.C_HUF20, 0x24) == A.E_UNSUPPORTED
    assert compress(A.C_LZ77, A.LZ77_HUF20_4) == A.E_UNSUPPORTED and compress(A.C_LZ77, A.LZ77_HUF20_8) == A.E_UNSUPPORTED
    assert compress(A.C_LEVEL5, A.LEVEL5_HUFFMAN4) == A.E_UNSUPPORTED and compress(A.C_LEVEL5, A.LEVEL5_HUFFMAN8) == A.E_UNSUPPORTED
    assert compress(A.C_LEVEL5, A.LEVEL5_HUFFMAN4, quality=0) == A.E_INVALID   # quality 0 -> OnlySave keeps precedence: the call gets as far as its missing context
    assert compress(A.C_LZ77, A.LZ77_RLE30) == A.E_INVALID and compress(A.C_RLE30, 0) == A.E_INVALID
    from auroralib.compression_amd import formats as F
    for obj, t in ((F.HUF20(), F.HUF20.Huffman4bits), (F.HUF20(), F.HUF20.Huffman8bits), (F.LZ77(), F.LZ77.HUF20_4bits), (F.LZ77(), F.LZ77.HUF20_8bits),
                   (F.Level5(), F.Level5.Huffman4Bit), (F.Level5(), F.Level5.Huffman8Bit)):
        obj.Type = t
        with pytest.raises(NotImplementedError, match="unstable"):
            obj.Compress(b"abcdabcd")
    assert F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20] and (F.LZ77.RLE30, F.Level5.RLE) == (0x30, 4)


def test_rlh_kernels_use_no_scratch_and_do_not_spill(tmp_path):
    k = {n: v for n, v in MC._kernel_notes(tmp_path).items() if "alz_rlh" in n}
    assert len(k) >= 5, sorted(k)                    # RLE30 decode x 2 families, RLE30 encode, HUF20 decode 4- and 8-bit
    for n, v in k.items():
        print("%s: %d VGPRs, %d B LDS" % (n, v["vgpr_count"], v["group_segment_fixed_size"]))
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (n, v)


def test_kernel_hash_lists_the_family():
    spec = importlib.util.spec_from_file_location("alz_kernel_hash_r", os.path.join(ROOT, "tools", "kernel_hash.py"))
    kh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kh)
    assert sorted(kh.FAMILIES["rlh"]) == ["alz_rlh.h", "alz_rlh.hip"]
    for fam in ("decode", "encode", "measure"):
        assert not any(f.startswith("alz_rlh") for f in kh.family_files(fam)), fam
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_rlh.hip" in build
