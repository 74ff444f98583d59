"""No GPU: what csrc/alz_framing.h makes of an LZ4 or Snappy file once the results of its bodies are known -- the rules the single-file measure, the
single-file Snappy decode and the two batched file calls share -- as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/framing_replay_check.cpp, `make -C oracle framing_replay_check`).  The CPU oracle stands in for the GPU: it decodes every body by itself
(O.decode_stream, without a bound, and for the decode side of a Snappy file with the capacities the layout asks for), the program turns those
results into the file's verdict, and the verdict is compared with the oracle's in-order reader on the whole file (oracle_container_decompress)
at the same capacity: rc always; status and dst_len when rc is ALZ_OK or ALZ_E_STREAM; src_used when the status is OK -- the rule of compare()
in tests/test_gpu_framed_decode.py.  No pair is left out.  The one documented deviation -- the library refuses a Snappy chunk whose body does
not end at its declared length, the oracle reads on -- is decided from the oracle alone (framing_cases.snappy_refusal_reached), and for such
a pair the decode side has to answer ALZ_E_FORMAT.

The sanitized binary is started directly and nothing here sets LD_PRELOAD (tests/test_framing_walk_cpu.py says why)."""
import os
import subprocess

import framing_cases as FC
import oracle_lib as O
import test_framing_walk_cpu as W
import test_gpu_framed_decode as GD
from auroralib.compression_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oracle", "framing_replay_check")
CASES = W.CASES
NO_BOUND = 0xFFFFFF00


def oracle_outcome(container, data, cap):
    """(rc, status, dst_len, src_used, bytes) of the oracle's in-order reader"""
    return GD.oracle_decode(GD.CT[container], bytes(data), cap)


# ------------------------------------------------------------------------------------------------ body results from the oracle


def lz4_body(cache, data, off, n):
    """An LZ4 block measured without a bound: no block decodes to more than 255 times its length."""
    key = bytes(data[off:off + n])
    if key not in cache:
        _, r = O.decode_stream(A.FMT_LZ4_BLOCK, key, cap=min(NO_BOUND, (16 << 20) + 4096))
        if r.status == A.ST_OUTPUT_CAPACITY:
            _, r = O.decode_stream(A.FMT_LZ4_BLOCK, key, cap=min(NO_BOUND, 255 * n + 4096))
        cache[key] = "%d:%d:%d" % (r.status, r.dst_len, r.src_used)
    return cache[key]


def snappy_chunk(data, pos):
    """The chunk header at pos as the reader of csrc/alz_framing.h returns it: (kind, body, declared length, stored bytes, next)."""
    n = len(data)
    if pos + 4 > n:
        return "truncated", pos, 0, 0, pos
    typ, cl = data[pos], int.from_bytes(data[pos + 1:pos + 4], "little")
    body = pos + 4
    nxt = min(pos + 4 + cl, n)
    if typ <= 1:
        if body + 4 > n or (typ == 1 and cl < 4):
            return "truncated", body, cl, 0, body
        body += 4
        return ("compressed", body, cl, 0, nxt) if typ == 0 else ("stored", body, cl, min(cl - 4, n - body), nxt)
    if typ <= 0x7F:
        return "reserved", body, cl, 0, body
    return "skipped", body, cl, 0, nxt


def snappy_declared_size(data, pos):
    v, shift, b = 0, 0, 0x80
    while b & 0x80 and pos < len(data):
        b = data[pos]
        pos += 1
        if shift < 32:
            v |= (b & 0x7F) << shift
        shift += 7
    return v & 0xFFFFFFFF


def snappy_results(data, cap, unbounded):
    """The results the program may ask for at this capacity, as "<body offset>:<dst_cap>:<status>:<dst_len>:<src_used>".  `unbounded` caches the
    measured bodies of this file."""
    found = {}

    def body(off, room):
        if (off, room) not in found:
            if room != NO_BOUND:
                found[(off, room)] = O.decode_stream(A.FMT_SNAPPY_RAW, data[off:], cap=room)[1]
            else:
                if off not in unbounded:
                    # a body stops once it has produced its declared size; its last element adds 64 bytes or a literal the input holds
                    rest = len(data) - off
                    unbounded[off] = O.decode_stream(A.FMT_SNAPPY_RAW, data[off:], cap=min(snappy_declared_size(data, off) + rest + 64, 32 * rest + 64))[1]
                found[(off, room)] = unbounded[off]
        return found[(off, room)]

    def declared(pos):
        while pos < len(data):
            kind, at, _, _, nxt = snappy_chunk(data, pos)
            if kind in ("truncated", "reserved"):
                return
            if kind == "compressed":
                yield at
            pos = nxt

    # a measure: the bodies at the declared places, and from wherever the in-order reader leaves them
    for off in declared(10):
        body(off, NO_BOUND)
    pos = 10
    while pos < len(data):
        kind, at, _, _, nxt = snappy_chunk(data, pos)
        if kind in ("truncated", "reserved"):
            break
        if kind == "compressed":
            if (at, NO_BOUND) not in found:
                for off in declared(pos):
                    body(off, NO_BOUND)
            r = body(at, NO_BOUND)
            if r.status != A.ST_OK:
                break
            nxt = at + r.src_used
        pos = nxt
    # a decode: every chunk at its declared place, clipped to the destination ...
    pos, out = 10, 0
    while pos < len(data):
        kind, at, _, stored, pos = snappy_chunk(data, pos)
        if kind in ("truncated", "reserved"):
            break
        if kind == "compressed":
            size = snappy_declared_size(data, at)
            body(at, min(cap - out, size) if out < cap else 0)
            out += size
        out += stored
    # ... and in order, with all the room that is left
    pos, out = 10, 0
    while pos < len(data):
        kind, at, cl, stored, nxt = snappy_chunk(data, pos)
        if kind in ("truncated", "reserved") or out + stored > cap:
            break
        if kind == "compressed":
            r = body(at, min(max(cap - out, 0), 0xFFFFFFFF))
            if r.status != A.ST_OK or r.src_used + 4 != cl:
                break
            out += r.dst_len
            nxt = at + r.src_used
        out += stored
        pos = nxt
    return ["%d:%d:%d:%d:%d" % (off, room, r.status, r.dst_len, r.src_used) for (off, room), r in found.items()]


# ------------------------------------------------------------------------------------------------ the program


def may_carry_content_checksum(data):
    """a frame magic with FLG bit 2 behind it, anywhere in the file"""
    k = data.find(b"\x04\x22\x4d\x18")
    while k >= 0:
        if k + 4 < len(data) and data[k + 4] & 4:
            return True
        k = data.find(b"\x04\x22\x4d\x18", k + 1)
    return False


def replay(pairs, tmp_path):
    """pairs: (container, data, capacity), the pairs of one file next to each other.  Returns the program's verdicts: per pair a list of
    (rc, status, dst_len, src_used) -- one for an LZ4 file, two (as a measure, as a decode) for a Snappy file."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "framing_replay_check"], stdout=subprocess.DEVNULL)
    lz4_files = []
    for container, data, _ in pairs:
        if container != "snappy" and (not lz4_files or lz4_files[-1][1] is not data):
            lz4_files.append((container, data))
    rc, lines, n = W.walk(lz4_files, tmp_path)                                     # the blocks of every LZ4 file, as the readers find them
    assert rc == 0 and len(lines) == n == len(lz4_files), (rc, lines[-3:])
    blocks = {id(data): [b for rec in W.parse(line)[2] for b in rec[7]] for (_, data), line in zip(lz4_files, lines)}
    src, out = str(tmp_path / "replay_inputs.txt"), str(tmp_path / "replay_output.txt")
    bodies, previous, unbounded, decoded = {}, None, {}, "-"
    with open(src, "w") as fh:
        for container, data, cap in pairs:
            same = previous is data
            if not same:
                previous, unbounded = data, {}
                # the decoded bytes, where a frame may carry a content checksum (FLG bit 2 is never mutated: the files of six cases)
                decoded = (oracle_outcome(container, data, len(data) * 255 + (1 << 16))[4].hex() or "-") if may_carry_content_checksum(data) else "-"
            if container == "snappy":
                words = snappy_results(data, cap, unbounded)
            else:
                words = [decoded] + [lz4_body(bodies, data, off, n_) for off, n_, raw, _ in blocks[id(data)] if not raw]
            fh.write("%s %d %s %s\n" % (container, cap, "=" if same else (bytes(data).hex() or "-"), " ".join(words)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:exitcode=77", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    with open(src) as fi, open(out, "w") as fo:
        p = subprocess.run([EXE], stdin=fi, stdout=fo, stderr=subprocess.STDOUT, env=env, timeout=900)
    lines = open(out).read().splitlines()
    assert p.returncode == 0 and len(lines) == len(pairs), (p.returncode, lines[-3:])
    verdicts = []
    for line in lines:
        v = [int(x) for x in line.split()]
        verdicts.append([tuple(v[k:k + 4]) for k in range(0, len(v), 4)])
    return verdicts


def difference(got, want, where):
    """the first difference between a verdict and the oracle's, or None"""
    if got[0] != want[0]:
        return "%s: rc %d, oracle %d (status %d / %d)" % (where, got[0], want[0], got[1], want[1])
    if got[0] in (0, A.E_STREAM) and got[1:3] != want[1:3]:
        return "%s: status/dst_len %d/%d, oracle %d/%d" % (where, got[1], got[2], want[1], want[2])
    if got[0] in (0, A.E_STREAM) and got[1] == A.ST_OK and got[3] != want[3]:
        return "%s: src_used %d, oracle %d" % (where, got[3], want[3])
    return None


def check(pairs, tmp_path):
    """Every pair through the program and against the oracle; returns (differences, Snappy pairs, Snappy pairs that reach the refusal)."""
    bad, snappy, refused = [], 0, 0
    for (container, data, cap), verdict in zip(pairs, replay(pairs, tmp_path)):
        want = oracle_outcome(container, data, cap)[:4]
        where = "%s, %d bytes, cap=%d" % (container, len(data), cap)
        assert len(verdict) == (2 if container == "snappy" else 1), where
        bad.append(difference(verdict[0], want, where + (" (measure)" if container == "snappy" else "")))
        if container == "snappy":
            snappy += 1
            if FC.snappy_refusal_reached(data, cap):
                refused += 1
                bad.append(None if verdict[1][0] == A.E_FORMAT else "%s (decode): rc %d where the refusal is reached" % (where, verdict[1][0]))
            else:
                bad.append(difference(verdict[1], want, where + " (decode)"))
    return [e for e in bad if e], snappy, refused


def test_generated_cases_at_every_capacity(tmp_path):
    """The 41 generated files at ample, exact, one-short, zero and mid-block capacity."""
    pairs = []
    for case in CASES:
        rng = FC.random.Random(case.seed)
        pairs += [(case.container, case.data, cap) for cap in GD.capacities(case, rng, len(case.expect))]
    bad, snappy, refused = check(pairs, tmp_path)
    assert not bad, (len(bad), bad[:8])
    assert len(CASES) == 41 and snappy >= 28 and refused == 0


def test_lz4_prefixes_cut_at_field_boundaries(tmp_path):
    """The 34 LZ4 files cut at the start and the end of every field the generator recorded, at ample capacity."""
    pairs = []
    for case in CASES:
        if case.container != "snappy":
            bounds = {fl[1] for fl in case.fields} | {fl[1] + fl[2] for fl in case.fields}
            pairs += [(case.container, case.data[:cut], len(case.expect) + 4096) for cut in sorted(bounds)]
    assert sum(c.container != "snappy" for c in CASES) == 34 and len(pairs) > 34 * 8
    bad, _, _ = check(pairs, tmp_path)
    assert not bad, (len(bad), bad[:8])


def test_mutants_at_ample_exact_one_short_and_zero_capacity(tmp_path):
    """The seeded mutants the GPU test decodes, at ample capacity, at what the oracle delivers there, at one byte less and at zero."""
    pairs = []
    for i, case in enumerate(CASES):
        for mu in FC.mutants(case, FC.SEED * 7919 + i):
            ample = len(case.expect) + (1 << 20)
            n = oracle_outcome(mu.container, mu.data, ample)[2]
            pairs += [(mu.container, mu.data, cap) for cap in sorted({ample, n, max(n - 1, 0), 0})]
    bad, snappy, refused = check(pairs, tmp_path)
    print("mutant pairs: %d, Snappy: %d, of them reaching the refused chunk: %d" % (len(pairs), snappy, refused))
    assert not bad, (len(bad), bad[:8])
    assert refused > 0                                                             # the branch is exercised
