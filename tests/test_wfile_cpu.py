"""No GPU: the wrapped-file layer (alz_wfile_*).  Declarations, exported symbols and ctypes prototypes; is_match / decompressed_size / walk of the
built library against the field lists that the builders of tests/wfile_ref.py record; every prefix and 200 seeded single-byte mutants per kind;
the library's SSZL keystream against its Python restatement; the same files, prefixes and mutants through the walks in a stand-alone program built
with -fsanitize=address,undefined (tests/wfile_walk_check.cpp: started in the test's own environment, nothing sets or edits LD_PRELOAD)."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import test_measure_cpu as MC
import test_shim_binding as SB
import wfile_ref as W
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(A.WFILE_PROTOTYPES)


def _lib():
    from auroralib.compression_amd._lib import load
    return load()


def walk(kind, big, data):
    """(rc, parts, stated, flags) as the library answers"""
    lib = _lib()
    o = A.ContainerOptions()
    o.big_endian = big
    n, size, fl = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = lib.alz_wfile_walk(kind, C.byref(o), data, len(data), None, 0, C.byref(n), C.byref(size), C.byref(fl))
    parts = (A.WfilePart * max(n.value, 1))()
    if rc == A.E_INVALID and n.value:
        need = n.value
        if need > 1:                                                  # one slot short: still ALZ_E_INVALID with the count needed
            assert lib.alz_wfile_walk(kind, C.byref(o), data, len(data), parts, need - 1, C.byref(n), C.byref(size), C.byref(fl)) == A.E_INVALID and n.value == need
        rc = lib.alz_wfile_walk(kind, C.byref(o), data, len(data), parts, need, C.byref(n), C.byref(size), C.byref(fl))
    return rc, [(p.src_off, p.src_len, p.body, p.dst_len) for p in parts[:n.value]], size.value, fl.value


def size_of(kind, big, data):
    o, v = A.ContainerOptions(), C.c_uint32(0xDEAD)
    o.big_endian = big
    return _lib().alz_wfile_decompressed_size(kind, C.byref(o), data, len(data), C.byref(v)), v.value


def clean():
    return [c for c in W.corpus() if c[4] is not None]


def one_per_kind():
    seen, out = set(), []
    for c in clean():
        if c[1] not in seen and not (c[1] == W.HWGZ and "5 chunks" not in c[0]) and not (c[1] == W.ZLWF and "3 chunks" not in c[0]):
            seen.add(c[1]); out.append(c)
    assert len(out) == 8
    return out


def variants():
    """(kind, big, bytes): the corpus, every prefix of one file per kind, 200 seeded single-byte mutants per kind"""
    out = [(c[1], c[2], c[3]) for c in W.corpus()]
    for name, kind, big, f, _, _, _ in one_per_kind():
        out += [(kind, big, f[:k]) for k in range(len(f))]
        rng = random.Random(1000 + kind)
        for _ in range(200):
            b = bytearray(f)
            at = rng.randrange(min(len(b), 160)) if rng.random() < 0.7 else rng.randrange(len(b))     # most of them in the headers and tables
            b[at] = rng.choice([0, 0xFF, b[at] ^ (1 << rng.randrange(8)), rng.randrange(256)])
            out.append((kind, big, bytes(b)))
    return out


def test_header_and_python_declare_the_entry_points():
    protos, types = SB._header_prototypes(), MC._header_types()
    for name in NAMES:
        py = A.WFILE_PROTOTYPES[name]
        assert protos.get(name) == len(py), name
        for ct, pt in zip(types.get(name, ()), py):           # (the helper reads the functions that return int)
            want = {"uint32_t": C.c_uint32, "size_t": C.c_size_t, "int": C.c_int}.get(ct)
            assert (pt is want) if want else (ct.endswith("*") and pt is not C.c_uint32 and pt is not C.c_size_t), (name, ct, pt)
    hdr = open(SB.HDR).read()
    enum = re.search(r"typedef enum alz_wfile_kind \{([^}]*)\}", hdr).group(1)
    assert [s.strip().split(" ")[0] for s in enum.split(",")] == ["ALZ_WF_" + n.upper() for n in A.WF_NAMES] + ["ALZ_WF_COUNT"]
    assert (A.WF_ASURAZLB, A.WF_RLHUDSON, A.WF_COUNT) == (0, 7, 8) and C.sizeof(A.WfilePart) == 16
    assert not [l for l in hdr.splitlines() if "NOT BUILT" in l and "Extended" in l]
    # the pinned constants are unchanged
    assert re.search(r"#define ALZ_ABI_VERSION 2\b", hdr) and (A.ABI_VERSION, A.RLH_COUNT, A.C_COUNT, A.FMT_COUNT) == (2, 3, 46, 25)
    assert F.ALL_FORMATS[-2:] == [F.RLE30, F.HUF20] and not set(F.WRAPPED_FORMATS) & set(F.ALL_FORMATS)
    assert [c.__name__ for c in F.WRAPPED_FORMATS] == ["AsuraZlb", "ZLB", "MDF0", "RareZip", "HWGZ", "SSZL", "ZLWF", "RLHudson"]
    assert [c.kind for c in F.WRAPPED_FORMATS] == list(range(8))
    from auroralib.compression_amd.batch import Context
    assert callable(Context.wfile_decode_batch)


def test_library_exports_the_entry_points():
    so = os.path.join(ROOT, "auroralib", "compression_amd", "libauroralz.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(_lib(), name).argtypes == A.WFILE_PROTOTYPES[name]
    build = open(os.path.join(ROOT, "auroralib", "compression_amd", "csrc", "build.sh")).read()
    assert "alz_wfile.cpp" in build


def test_walk_reports_the_builders_fields():
    for name, kind, big, f, want, data, expect in clean():
        assert _lib().alz_wfile_is_match(kind, f, len(f)) == 1, name
        assert size_of(kind, big, f) == (0, want["stated"]), name
        rc, parts, stated, flags = walk(kind, big, f)
        assert (rc, parts, stated, flags) == (0, want["parts"], want["stated"], want["flags"]), name
    names = " | ".join(c[0] for c in W.corpus())
    for need in ("hwgz 1 chunks", "hwgz 2 chunks", "hwgz 5 chunks", "header little, order big", "zlwf 1 chunks big", "zlwf 3 chunks little", "gzip",
                 "options 0x0,", "options 0x1,", "options 0x80000000,", "options 0x80000001,", "= 0 mod 4", "= 1 mod 4", "= 2 mod 4", "= 3 mod 4"):
        assert need in names, need
    for cls in F.WRAPPED_FORMATS:                                     # ... and through the Python classes
        c = next(c for c in clean() if c[1] == cls.kind and c[2] == (1 if cls in (F.HWGZ, F.ZLWF) else 0))
        obj = cls()
        assert obj.IsMatch(c[3]) and obj.GetDecompressedSize(c[3]) == c[4]["stated"] and obj.Walk(c[3]) == (c[4]["parts"], c[4]["stated"], c[4]["flags"])


def test_is_match_length_rules():
    m = lambda kind, data: _lib().alz_wfile_is_match(kind, bytes(data), len(data))
    z = bytes.fromhex("789c4b4c4a0600024d0127")
    assert m(W.ASURAZLB, b"AsuraZlb" + bytes(13)) == 1 and m(W.ASURAZLB, b"AsuraZlb" + bytes(12)) == 0          # more than 0x14 bytes
    assert m(W.ZLB, b"ZLB\0" + bytes(17)) == 1 and m(W.ZLB, b"ZLB\0" + bytes(16)) == 0                            # 0x14 behind a 16-byte header
    assert m(W.MDF0, b"mdf\0\5\0\0\0" + z) == 1 and m(W.MDF0, b"mdf\0\0\0\0\0" + z) == 0 and m(W.MDF0, b"mdf\0\5\0\0\0" + b"\x79" + z[1:]) == 0
    assert m(W.MDF0, (b"mdf\0\5\0\0\0" + z)[:16]) == 0 and m(W.MDF0, (b"mdf\0\5\0\0\0" + z)[:17]) == 1
    assert m(W.RAREZIP, b"\x11\x72\0\0\0\1\0") == 1 and m(W.RAREZIP, b"\x11\x72\0\0\0\1") == 0 and m(W.RAREZIP, b"\x11\x72\0\0\0\0\0") == 0
    assert m(W.SSZL, b"SSZL" + struct.pack("<I", 0x20101109) + bytes(9)) == 1 and m(W.SSZL, b"SSZL" + struct.pack("<I", 0x20101109) + bytes(8)) == 0
    assert m(W.SSZL, b"SSZL" + struct.pack("<I", 0x20101108) + bytes(9)) == 0
    assert m(W.ZLWF, b"ZLWF" + bytes(13)) == 1 and m(W.ZLWF, b"ZLWF" + bytes(12)) == 0
    assert m(W.RLHUDSON, struct.pack(">II", 9, 5)) == 1 and m(W.RLHUDSON, struct.pack(">II", 0, 5)) == 0 and m(W.RLHUDSON, struct.pack(">II", 9, 4)) == 0
    assert m(W.RLHUDSON, struct.pack(">II", 9, 5)[:7]) == 0
    f = W.hwgz(W.sample(100, 3), 64)[0]
    assert len(f) >= 0x80 and m(W.HWGZ, f) == 1 and m(W.HWGZ, f[:0x7F]) == 0
    assert m(W.HWGZ, f[:132] + b"\x79" + f[133:]) == 0                 # ZLib.IsMatchStatic four bytes behind the aligned table
    assert m(99, f) == 0
    # wrong magic: ALZ_E_FORMAT; a header that runs past the input: ALZ_E_STREAM
    assert walk(W.ZLB, 0, b"ZLC\0" + bytes(20))[0] == A.E_FORMAT and walk(W.ZLB, 0, b"ZLB\0" + bytes(8))[0] == A.E_STREAM and walk(W.ZLB, 0, b"ZL")[0] == A.E_STREAM
    assert walk(W.HWGZ, 1, struct.pack(">III", 64, 3, 100) + bytes(200))[0] == A.E_FORMAT                        # validates in neither order
    assert walk(W.HWGZ, 1, struct.pack(">III", 1, 0x1000, 0x1000) + bytes(200))[0] == A.E_STREAM                 # more chunks than the file can hold
    zl = W.zlwf(W.sample(100, 4), 64)[0]
    assert walk(W.ZLWF, 1, zl[:32] + b"WFLX" + zl[36:])[0] == A.E_FORMAT and walk(W.ZLWF, 1, zl[:12] + struct.pack(">I", 1 << 20) + zl[16:])[0] == A.E_STREAM
    assert walk(W.ZLWF, 1, zl[:16] + struct.pack(">I", len(zl)) + zl[20:])[0] == A.E_STREAM
    assert walk(99, 0, zl)[0] == A.E_INVALID


def test_prefixes_and_mutants_stay_inside_the_file():
    seen = set()
    for kind, big, f in variants():
        rc, parts, stated, flags = walk(kind, big, f)
        assert rc in (0, A.E_FORMAT, A.E_STREAM), (kind, len(f), rc)
        seen.add(rc)
        for off, ln, body, dl in parts:
            assert off + ln <= len(f) and body <= A.WB_PLAIN, (kind, len(f), off, ln)
        assert _lib().alz_wfile_is_match(kind, f, len(f)) in (0, 1)
        assert size_of(kind, big, f)[0] in (0, A.E_FORMAT, A.E_STREAM)
    assert seen == {0, A.E_FORMAT, A.E_STREAM}


def test_a_null_context_is_refused_only_once_a_body_must_be_decoded():
    lib = _lib()
    dst = (C.c_uint8 * 4096)()
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    call = lambda kind, f: lib.alz_wfile_decompress(None, kind, None, f, len(f), dst, 4096, C.byref(dl), C.byref(su), C.byref(st))
    f = W.zlb(W.sample(300, 5))[0]
    assert call(W.ZLB, b"ZLX\0" + f[4:]) == A.E_FORMAT
    assert call(W.ZLB, f[:10]) == A.E_STREAM and st.value == A.ST_INPUT_TRUNCATED and su.value == 10
    assert call(W.ZLB, f) == A.E_INVALID
    assert call(99, f) == A.E_INVALID
    cdl = C.c_size_t()
    assert lib.alz_wfile_compress(None, W.ZLB, None, None, 6, 0, b"abc", 3, dst, 4096, C.byref(cdl)) == A.E_INVALID


def checker(tmp_path):
    """tests/wfile_walk_check.cpp built with g++ -fsanitize=address,undefined.  It is started directly, in the environment this test runs in:
    nothing here sets or edits LD_PRELOAD (on a host that preloads something into every command the sanitizer's runtime does not come first, the
    binary refuses to start and the test fails, as tests/test_framing_walk_cpu.py says of its own)."""
    exe = str(tmp_path / "wfile_walk_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "auroralib", "compression_amd", "csrc"), os.path.join(ROOT, "tests", "wfile_walk_check.cpp"), "-o", exe], check=True)
    return exe


def test_keystream_700_words(tmp_path):
    """The library's keystream -- alz_zfile.h's SszlTwister, the code the file layer XORs with, printed by the stand-alone program under the
    sanitizers -- against the restatement: 700 words cross the 624-word state.  Then the tail of 1-3 bytes, which takes one more word, in the
    builder, and the first word as the walk itself draws it to tell gzip from zlib behind the XOR.  (A decode of an encrypted file through the
    library compares the same 700 words once more: tests/test_gpu_wfile.py::test_keystream_700_words.)"""
    want = W.sszl_keystream(700)
    assert want[:3] == [439895749, 1892632068, 1788751189] and all(w < 1 << 31 for w in want)
    r = subprocess.run([checker(tmp_path), "--keystream", "700"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert [int(l) for l in r.stdout.split()] == want
    for tail in (0, 1, 2, 3):
        n = 2800 + tail
        f = W.sszl(bytes(n), W.ENCRYPTED)[0]
        rc, parts, stated, flags = walk(W.SSZL, 0, f)
        assert (rc, parts, stated, flags) == (0, [(20, n, A.WB_PLAIN, 0)], n, W.ENCRYPTED)
        assert f[20:] == b"".join(struct.pack("<I", w) for w in W.sszl_keystream(701))[:n]
    gz = W.sszl(W.sample(200, 6), W.COMPRESSED | W.ENCRYPTED, True)[0]
    assert walk(W.SSZL, 0, gz)[1][0][2] == A.WB_GZIP and walk(W.SSZL, 0, W.sszl(W.sample(200, 6), W.COMPRESSED | W.ENCRYPTED)[0])[1][0][2] == A.WB_ZLIB


def test_walks_under_address_and_undefined_sanitizers(tmp_path):
    """the walks over the same files, prefixes and mutants in the stand-alone program; what they answer is compared with the library's answers"""
    exe, corpus = checker(tmp_path), str(tmp_path / "corpus.bin")
    recs = variants()
    with open(corpus, "wb") as fh:
        fh.write(struct.pack("<I", len(recs)))
        for kind, big, f in recs:
            rc, parts, stated, flags = walk(kind, big, f)
            fh.write(struct.pack("<III", kind, big, len(f)) + f + struct.pack("<iIIIi", rc, len(parts), stated, flags, _lib().alz_wfile_is_match(kind, f, len(f))))
            for p in parts:
                fh.write(struct.pack("<IIII", *p))
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "%d records, 0 differ" % len(recs) in r.stdout
