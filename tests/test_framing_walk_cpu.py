"""No GPU: the LZ4 / Snappy framing readers of csrc/alz_framing.h -- the one walk behind the file decode and the file measure -- as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer (tests/framing_walk_check.cpp, `make -C oracle framing_walk_check`).  What the readers
return is compared with the field lists the generator of tests/framing_cases.py recorded while it wrote the files, and the readers are run to the end
of every generated file, every prefix around a field boundary and every seeded mutant.

The sanitized binary is started directly and nothing here sets LD_PRELOAD: the test is meant for hosts that preload nothing into every command (a
sanitizer's runtime has to come first in the library list, so on a host that does the binary refuses to start and the test fails)."""
import os
import struct
import subprocess
import sys

import framing_cases as FC
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "framing_walk_check")
CASES = FC.generated_cases(O.xxh32)


def walk(inputs, tmp_path):
    """Runs the binary over (container, bytes) inputs; returns (exit status, output lines, number of inputs).  Input and output go through files:
    the inputs are large."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "framing_walk_check"], stdout=subprocess.DEVNULL)
    src, out = str(tmp_path / "inputs.txt"), str(tmp_path / "output.txt")
    n = 0
    with open(src, "w") as fh:
        for container, data in inputs:
            fh.write("%s %s\n" % (container, bytes(data).hex()))
            n += 1
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:exitcode=77", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    with open(src) as fi, open(out, "w") as fo:
        p = subprocess.run([EXE], stdin=fi, stdout=fo, stderr=subprocess.STDOUT, env=env, timeout=900)
    return p.returncode, open(out).read().splitlines(), n


def parse(line):
    """One output line -> (container, length, [records]); an LZ4 record is (kind, flg, nominal, content, truncated, fault, end, [(off, len, raw, next)]),
    a Snappy record (kind, hdr, body, len, stored, next)."""
    head, *parts = line.split(" | ")
    h = head.split()
    recs = []
    for part in parts:
        t = part.split()
        if h[0] == "snappy":
            recs.append((t[0],) + tuple(int(x) for x in t[1:]))
        else:
            recs.append((t[0],) + tuple(int(x) for x in t[1:7]) + ([tuple(int(x) for x in b.split(":")) for b in t[7:]],))
    return h[0], int(h[1]), recs


def test_readers_return_the_structure_the_generator_recorded(tmp_path):
    rc, lines, n = walk([(c.container, c.data) for c in CASES], tmp_path)
    assert rc == 0 and len(lines) == n == len(CASES), (rc, lines[-3:])
    for case, line in zip(CASES, lines):
        container, length, recs = parse(line)
        assert (container, length) == (case.container, len(case.data)), case
        fl = case.fields
        if case.container == "snappy":
            want = []
            for i, (kind, off, n_, typ) in enumerate(fl):
                if kind != "chunk":
                    continue
                declared = int.from_bytes(case.data[off + 1:off + 4], "little")
                body = fl[i + 2][1] if typ < 0x80 else fl[i + 1][1]                # behind the CRC: the varint (compressed) or the body (stored)
                assert fl[i + 1][0] == ("crc" if typ < 0x80 else "body") and fl[i + 2 if typ < 0x80 else i + 1][0] in ("varint", "body"), case
                want.append(({0: "compressed", 1: "stored"}.get(typ, "skipped"), off, body, declared, declared - 4 if typ == 1 else 0, off + 4 + declared))
            assert recs == want, case
            continue
        frames = [r for r in recs if r[0] in ("legacy", "frame")]
        assert len(frames) == sum(1 for f in fl if f[0] == "magic"), case
        assert all(r[4] == 0 and r[5] == 0 for r in recs), case                     # truncated, fault
        want = []
        for i, (kind, off, n_, _) in enumerate(fl):
            if kind not in ("size", "lsize"):
                continue
            assert fl[i + 1][0] == "body", case
            word = int.from_bytes(case.data[off:off + 4], "little")
            _, boff, blen, _ = fl[i + 1]
            has_sum = i + 2 < len(fl) and fl[i + 2][0] == "bsum"
            want.append((boff, blen, int(kind == "size" and word >> 31), boff + blen + (4 if has_sum else 0)))
        assert [b for r in recs for b in r[7]] == want, case
        for r in frames:                                                            # header fields as the generator wrote them
            if r[0] == "frame":
                at = min(b[0] for b in r[7]) if r[7] else None
                flg = [f for f in fl if f[0] == "flg" and (at is None or f[1] < at)][-1]
                assert (r[1], r[2]) == (case.data[flg[1]], FC.BMAX[case.data[flg[1] + 1] >> 4]), case


def many_tiny_frames(n=65536):
    """1 MiB of 16-byte frames with one stored one-byte block each: what a reader keeps per FRAME must not grow with the rest of the file."""
    desc = bytes([0x40, 0x70])
    one = struct.pack("<I", 0x184D2204) + desc + bytes([(O.xxh32(desc) >> 8) & 0xFF]) + struct.pack("<I", 0x80000001) + b"x" + struct.pack("<I", 0)
    assert len(one) == 16
    return one * n


def test_many_tiny_frames_cost_memory_linear_in_the_file(tmp_path):
    """The program keeps every frame and one block list, as alz_container_measure does, and checks what they hold in the end against the file size."""
    data = many_tiny_frames()
    rc, lines, n = walk([("lz4", data), ("lz4", data[:-3])], tmp_path)
    assert rc == 0 and n == len(lines) == 2 and "VIOLATION" not in "".join(lines), (rc, [ln[-300:] for ln in lines])
    _, length, recs = parse(lines[0])
    assert length == len(data) and len(recs) == 65536
    assert all(r[:7] == ("frame", 0x40, 0x400000, 0, 0, 0, 16 * (i + 1)) and r[7] == [(16 * i + 11, 1, 1, 16 * i + 12)] for i, r in enumerate(recs))
    assert parse(lines[1])[2][-1][4] == 1                                           # the cut EndMark: truncated


def test_readers_stay_inside_every_prefix_and_mutant(tmp_path):
    """Every case, every prefix of it cut at a field boundary and one byte to either side of it, and every seeded mutant: the sanitizers and the
    program's own position checks stay silent, and every input gets its line."""
    def inputs():
        for i, case in enumerate(CASES):
            yield case.container, case.data
            bounds = {fl[1] for fl in case.fields} | {fl[1] + fl[2] for fl in case.fields}
            for cut in sorted({min(max(b + d, 0), len(case.data)) for b in bounds for d in (-1, 0, 1)}):
                yield case.container, case.data[:cut]
            for mu in FC.mutants(case, FC.SEED * 7919 + i, per_case=0):
                yield mu.container, mu.data
    rc, lines, n = walk(inputs(), tmp_path)
    text = "\n".join(lines[-40:])
    assert "AddressSanitizer" not in "\n".join(lines) and "runtime error" not in "\n".join(lines) and "VIOLATION" not in "\n".join(lines), text[-4000:]
    assert rc == 0, (rc, text[-4000:])
    assert len(lines) == n and n > 40 * len(CASES), (len(lines), n)


def test_kernel_hash_family():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_hash as KH
    assert KH.FAMILIES["framing"] == ["alz_framing.h"]
    for fam in KH.FAMILIES:
        assert ("alz_framing.h" in KH.family_files(fam)) == (fam == "framing"), fam
