"""-m gpu: RLHudson (alz_rlhudson_*) on the device.  Every case runs under the exact and the production context modes, through the host and
the device forms, and every result field and output byte is compared with the pure-Python restatement (tests/rlhudson_ref.py); the known answers
carry their expected results written out by hand.  Every destination of the device form has a canary on both sides."""
import random

import numpy as np
import pytest

import rlhudson_ref as W
from auroralib.compression_amd import _abi as A
from cases import prose_like
from gpu_common import ctx

pytestmark = pytest.mark.gpu
FAMILIES = ((1, "exact"), (0, "production"))
GUARD = 48
OFFS = (0, 1, 15, 17)                       # residues of dst_off mod 16: the granule write-back starts aligned, one in, one short, one over


# ---------------------------------------------------------------------------------------------- helpers
def run(n, b):
    return bytes([n, b])


def lit(data):
    return bytes([0x80 | len(data)]) + bytes(data)


def item(src, size, cap=None, name="", want=None):
    it = dict(src=bytes(src), decom_len=size, cap=size if cap is None else cap, name=name)
    if want is not None:
        ref = W.rlhudson_decode(it["src"], size, it["cap"])
        assert ref[:3] == want[:3] and (want[3] is None or ref[3] == want[3]), (name, ref, want)   # the hand-written answer pins the restatement
    it["want"] = W.rlhudson_decode(it["src"], size, it["cap"])
    return it


def pack(items, offs=OFFS):
    """stream i: source at residue i mod 16, destination at residue offs[i mod len(offs)] mod 16 with GUARD untouched bytes on both sides"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 0
    for i, it in enumerate(items):
        b, mis = it["src"], i % 16
        chunks.append(bytes(mis) + b + bytes((-(len(b) + mis)) % 16))
        do = (do + GUARD + 15) // 16 * 16 + offs[i % len(offs)]
        streams[i] = A.Stream(so + mis, do, len(b), it["cap"], it["decom_len"], 0, 0, 0)
        so += len(chunks[-1])
        do += it["cap"]
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + GUARD + 64


def compare(items, streams, res, dst, tag0):
    for i, it in enumerate(items):
        out, status, dst_len, src_used = it["want"]
        tag = "%s stream %d (%s)" % (tag0, i, it["name"])
        print("%s: gpu status=%d len=%d used=%d | ref status=%d len=%d used=%s" % (tag, res[i].status, res[i].dst_len, res[i].src_used, status, dst_len, src_used))
        assert (res[i].status, res[i].dst_len) == (status, dst_len), tag
        if src_used is not None:
            assert res[i].src_used == src_used, tag
        a = streams[i].dst_off
        got = dst[a:a + dst_len].tobytes()
        if got != out:
            d = next(k for k in range(dst_len) if got[k] != out[k])
            raise AssertionError("%s: byte %d of %d differs (gpu %d, ref %d)" % (tag, d, dst_len, got[d], out[d]))


def check_decode(items, what, offs=OFFS):
    """both context modes x (host form | device form with canaries)"""
    streams, src, dst_bytes = pack(items, offs)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        for exact, fam in FAMILIES:
            c.set_exact_kernels(exact)
            try:
                dst, res = c.rlhudson_decode_batch(streams, src, dst_bytes)
                compare(items, streams, res, dst, "%s [%s, host]" % (what, fam))
                c.memset(d_dst, 0xA5, dst_bytes)
                res = c.rlhudson_decode_batch_device(streams, d_src, src.nbytes - 64, d_dst, dst_bytes - 64)
            finally:
                c.set_exact_kernels(0)
            dst = c.d2h(d_dst, dst_bytes)
            compare(items, streams, res, dst, "%s [%s, device]" % (what, fam))
            touched = np.zeros(dst_bytes, dtype=bool)
            for i, it in enumerate(items):
                touched[streams[i].dst_off:streams[i].dst_off + it["want"][2]] = True      # dst_len bytes and nothing else
            bad = np.nonzero(~touched & (dst != 0xA5))[0]
            assert bad.size == 0, "%s [%s]: %d canary bytes changed, first at %d" % (what, fam, bad.size, bad[0])
    finally:
        c.free(d_src); c.free(d_dst)


# the production rounds run while 588 input bytes lie ahead: cases that are about a round carry this much behind them
TAIL = lit(bytes(range(90))) * 8


def tail_out():
    return bytes(range(90)) * 8


# ---------------------------------------------------------------------------------------------- known answers
def kat_items():
    OK, TR, MM, CAP = W.OK, W.INPUT_TRUNCATED, W.OUTPUT_SIZE_MISMATCH, W.OUTPUT_CAPACITY
    abc = bytes(range(0x41, 0x41 + 127))
    its = [
        item(run(5, 0x61), 5, name="a run", want=(b"aaaaa", OK, 5, 2)),
        item(lit(b"xyz"), 3, name="a literal run", want=(b"xyz", OK, 3, 4)),
        item(run(0, 9) + run(1, 0x62), 1, name="run of 0, run of 1", want=(b"b", OK, 1, 4)),
        item(run(127, 0x63), 127, name="run of 127", want=(b"c" * 127, OK, 127, 2)),
        item(lit(b"") + lit(b"d"), 1, name="0 literals, 1 literal", want=(b"d", OK, 1, 3)),
        item(lit(abc), 127, name="127 literals", want=(abc, OK, 127, 128)),
        item(b"\x80" * 256 + run(4, 0x65), 4, name="256 x 80, then a run", want=(b"eeee", OK, 4, 258)),
        item(b"\x80" * 256 + run(4, 0x65) + TAIL, 4 + 720, name="256 x 80, then a run, inside the rounds", want=(b"eeee" + tail_out(), OK, 724, 258 + len(TAIL))),
        item(run(0, 1) * 200 + lit(b"f") + TAIL, 1 + 720, name="200 runs of 0 (rounds that produce nothing)", want=(b"f" + tail_out(), OK, 721, 402 + len(TAIL))),
        item(b"".join(lit(bytes([k])) for k in range(128)) + TAIL, 128 + 720, name="128 one-literal tokens in one window",
             want=(bytes(range(128)) + tail_out(), OK, 848, 256 + len(TAIL))),
        item(run(3, 1), 10, name="ends at a control byte", want=(b"\1\1\1", TR, 3, 2)),
        item(run(3, 1) + b"\x05", 10, name="ends at a run byte", want=(b"\1\1\1", TR, 3, 3)),
        item(run(3, 1) + b"\x00", 10, name="ends at the byte of a run of 0", want=(b"\1\1\1", TR, 3, 3)),
        item(run(3, 1) + lit(b"abcd")[:-1], 10, name="ends inside a literal run", want=(b"\1\1\1", TR, 3, 6)),
        item(b"", 1, name="empty input", want=(b"", TR, 0, 0)),
        item(run(3, 1) + run(9, 2), 5, cap=64, name="overshoot of decom_len by a run", want=(b"\1\1\1" + b"\2" * 9, MM, 12, 4)),
        item(run(3, 1) + lit(b"abcdefg"), 5, cap=64, name="overshoot of decom_len by literals", want=(b"\1\1\1abcdefg", MM, 10, 10)),
        item(run(3, 1) + run(9, 2), 12, cap=7, name="dst_cap met inside a run", want=(b"\1\1\1\2\2\2\2", CAP, 7, None)),
        item(run(3, 1) + lit(b"abcdefg"), 10, cap=7, name="dst_cap met inside a literal run", want=(b"\1\1\1abcd", CAP, 7, None)),
        item(run(3, 1) + run(9, 2), 5, cap=7, name="dst_cap met by the overshooting token", want=(b"\1\1\1\2\2\2\2", MM, 7, 4)),
        item(run(3, 1), 0, name="decom_len 0", want=(b"", OK, 0, 0)),
        item(run(3, 1) + run(0, 7) + lit(b""), 3, name="empty elements behind the end are not read", want=(b"\1\1\1", OK, 3, 2)),
    ]
    return its


def test_known_answers():
    its = kat_items()
    check_decode(its, "kat")
    check_decode(its[1:] + its[:1], "kat, destinations moved on by one residue")       # every case at another of the four residues


def test_dst_cap_inside_the_rounds():
    """the token that meets dst_cap, and the one that overshoots decom_len, far enough from the end of the input that a round sees them"""
    body = (run(100, 3) + lit(bytes(range(100)))) * 4
    out = (b"\3" * 100 + bytes(range(100))) * 4
    its = []
    for cap in (0, 1, 99, 100, 101, 150, 199, 200, 201, 650, 799):
        its.append(item(body + TAIL, 800, cap=cap, name="cap %d of 800" % cap, want=(out[:cap], W.OUTPUT_CAPACITY, cap, None)))
    for size in (1, 99, 100, 101, 199, 200, 201, 790):
        end = -(-size // 100) * 100
        its.append(item(body + TAIL, size, cap=1000, name="declared %d" % size, want=(out[:end], W.OK if end == size else W.OUTPUT_SIZE_MISMATCH, end, None)))
    check_decode(its, "cap and size inside the rounds")


def fill(nbytes):
    """exactly `nbytes` (>= 2) input bytes of whole literal elements of at least two bytes, and what they decode to"""
    s, out, rest = b"", b"", nbytes
    while rest:
        size = rest if rest <= 101 else 100                            # (what is left behind a piece of 100 is at least 2)
        d = bytes((nbytes + rest + j) & 0xFF for j in range(size - 1))
        s += lit(d); out += d; rest -= size
    assert len(s) == nbytes
    return s, out


def test_elements_across_the_window_edge():
    """an element that straddles the edge of the first 256-byte window at each of its byte positions: the control byte is the window's last byte,
    ..., the element's last byte is the next window's first"""
    its = []
    for kind, el, out in (("run", run(9, 0x77), b"\x77" * 9), ("run of 0", run(0, 0x77), b""), ("5 literals", lit(b"hello"), b"hello"),
                          ("127 literals", lit(bytes(range(127))), bytes(range(127)))):
        for k in range(len(el) + 1):                                   # k bytes of the element lie inside the window
            front = 256 - k
            pre, want = fill(front)
            its.append(item(pre + el + TAIL, len(want) + len(out) + 720, name="%s, %d of its %d bytes inside the window" % (kind, k, len(el)),
                            want=(want + out + tail_out(), W.OK, len(want) + len(out) + 720, front + len(el) + len(TAIL))))
    check_decode(its, "window edge")


def test_long_streams():
    """streams of many input-cache chunks (512 bytes each), and the element counts around one round's 64"""
    its = []
    for ntok in (63, 64, 65):
        for kind in ("run1", "run0", "lit1", "mixed"):
            toks = [(run(1 if kind != "run0" else 0, 0x10 + k) if kind.startswith("run") or (kind == "mixed" and k & 1) else lit(bytes([k]))) for k in range(ntok)]
            s = b"".join(toks) + TAIL
            its.append(item(s, len(W.rlhudson_decode(s, 1 << 20, 1 << 20)[0]), name="%d x %s" % (ntok, kind)))
    its.append(item(run(127, 0xEE) * 300, 38100, name="all runs of 127"))
    its.append(item(b"".join(lit(bytes([k & 0xFF])) for k in range(2500)), 2500, name="all literals of 1"))
    its.append(item(b"".join(lit(bytes((k + j) & 0xFF for j in range(127))) + run(3, k & 0xFF) for k in range(150)), 150 * 130, name="127 literals / run of 3"))
    zeros = bytearray(65536)
    for k in range(0, 65536, 997):
        zeros[k] = 1 + k % 255
    for name, data in (("prose", prose_like(65536, 31)), ("mostly zero", bytes(zeros))):
        assert not W.rlhudson_has_defect(data)
        s = W.rlhudson_encode(data)
        its.append(item(s, len(data), name="64 KiB " + name, want=(data, W.OK, len(data), len(s))))
    assert sum(it["cap"] for it in its) < 300 << 10
    check_decode(its, "long streams")


# ---------------------------------------------------------------------------------------------- differential
def random_stream(rng, nbytes):
    """a valid RLHudson stream of random elements, empty ones included, that decodes to exactly its declared size"""
    s, out = bytearray(), bytearray()
    while len(out) < nbytes:
        room = nbytes - len(out)
        if rng.random() < 0.5:
            n, b = min(rng.choice([0, 1, 2, 3, 5, 17, 64, 65, 126, 127]), room), rng.randrange(256)
            s += run(n, b); out += bytes([b]) * n
        else:
            d = bytes(rng.randrange(256) for _ in range(min(rng.choice([0, 1, 1, 2, 3, 7, 63, 64, 65, 127]), room)))
            s += lit(d); out += d
    return bytes(s), bytes(out)


def differential_items():
    rng = random.Random(0x4855)
    its = []
    for k in range(300):
        s, out = random_stream(rng, rng.choice([0, 1, 7, 100, 600, 1000]) if k % 3 else rng.randrange(0, 8193))
        it = item(s, len(out), name="seeded %d" % k)
        assert it["want"][:3] == (out, W.OK, len(out))
        its.append(it)
    return its


def test_differential_300_streams():
    check_decode(differential_items(), "differential")


def test_differential_300_streams_cut():
    rng = random.Random(0x4856)
    its = []
    for it in differential_items():
        s = it["src"]
        its.append(item(s[:rng.randrange(len(s) + 1)], it["decom_len"], name=it["name"] + ", cut"))
    seen = {it["want"][1] for it in its}
    assert {W.OK, W.INPUT_TRUNCATED} <= seen
    check_decode(its, "differential, cut")


def test_noise_and_capacities():
    """random bytes as streams (every control byte, whatever follows), declared sizes and capacities on both sides of what they decode to"""
    rng = random.Random(0x4857)
    its = []
    for k in range(96):
        n = rng.choice([0, 1, 2, 63, 64, 129, 587, 588, 589, 1000, 1500, 4000])
        src = bytes(rng.choice([0, 0x80, 0x81, 0x7F, 0xFF, 1, rng.randrange(256), rng.randrange(256)]) for _ in range(n))
        decl = rng.choice([0, 1, 50, 400, 3000])
        cap = rng.choice([decl, decl + 300, max(decl, 1) // 2, decl - 1 if decl else 0])
        its.append(item(src, decl, cap=cap, name="noise %d" % k))
    seen = {it["want"][1] for it in its}
    print("statuses seen:", sorted(seen))
    assert {W.OK, W.INPUT_TRUNCATED, W.OUTPUT_CAPACITY, W.OUTPUT_SIZE_MISMATCH} <= seen
    check_decode(its, "noise")


# ---------------------------------------------------------------------------------------------- encode
def nonrepeating(n):
    """bytes without two equal neighbours: nothing for the run finder"""
    return bytes((7 * i + (i >> 8)) & 0xFF for i in range(n))


def encode_sets():
    sets = [("0", b""), ("1", b"a"), ("2", b"ab"), ("3", b"abc"), ("3 equal", b"aaa")]
    sets += [("run %d" % n, b"q" * n) for n in (2, 3, 127, 128, 130)]
    sets += [("nonrepeating %d" % n, nonrepeating(n)) for n in (126, 127, 128, 129, 130)]
    sets += [("ab + run + de", b"ab" + b"c" * 300 + b"de"), ("pairs", b"aabbccddee" * 40), ("triples", b"aaabbbcccdddeee" * 40), ("zeros", bytes(3000))]
    rng = np.random.default_rng(0x4858)
    for k in range(200):
        n = int(rng.integers(0, 1500))
        d = bytearray(prose_like(n, 300 + k))
        for _ in range(int(rng.integers(0, 6))):                       # some runs of every length class
            a, ln = int(rng.integers(0, max(n, 1))), int(rng.integers(2, 400))
            d[a:a + ln] = bytes([int(rng.integers(0, 256))]) * len(d[a:a + ln])
        sets.append(("seeded %d" % k, bytes(d)))
    return sets


def check_encode(named, what, short=False):
    """both context modes (one kernel serves both) x host and device form; short: dst_cap one byte below the need"""
    n = len(named)
    want = [W.rlhudson_encode(d) for _, d in named]
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 0
    for i, (_, d) in enumerate(named):
        cap = max(len(want[i]) - 1, 0) if short else (len(want[i]) if i % 2 else W.rlhudson_encode_bound(len(d)) + 8)
        do = (do + GUARD + 15) // 16 * 16 + OFFS[i % 4]
        streams[i] = A.Stream(so, do, len(d), cap, 0, 0, 0, 0)
        chunks.append(d + bytes((-len(d)) % 16))
        so += len(chunks[-1]); do += cap
    dst_bytes = do + GUARD + 64
    src = np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy()
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        for exact, fam in FAMILIES:
            c.set_exact_kernels(exact)
            try:
                h_dst, h_res = c.rlhudson_encode_batch(streams, src, dst_bytes)
                c.memset(d_dst, 0xA5, dst_bytes)
                d_res = c.rlhudson_encode_batch_device(streams, d_src, src.nbytes - 64, d_dst, dst_bytes - 64)
            finally:
                c.set_exact_kernels(0)
            dd = c.d2h(d_dst, dst_bytes)
            touched = np.zeros(dst_bytes, dtype=bool)
            for form, dst, res in (("host", h_dst, h_res), ("device", dd, d_res)):
                for i, (name, d) in enumerate(named):
                    tag = "%s [%s, %s] %s (%d bytes)" % (what, fam, form, name, len(d))
                    a = streams[i].dst_off
                    if len(want[i]) > streams[i].dst_cap:
                        assert (res[i].status, res[i].dst_len) == (A.ST_OUTPUT_CAPACITY, 0), tag
                        touched[a:a + streams[i].dst_cap] = True       # (what a failed encode left inside its capacity is unspecified)
                        continue
                    assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(want[i]), len(d)), tag
                    assert dst[a:a + len(want[i])].tobytes() == want[i], tag
                    touched[a:a + len(want[i])] = True
            assert not np.any(~touched & (dd != 0xA5)), "%s [%s]: a byte outside a stream's output changed" % (what, fam)
    finally:
        c.free(d_src); c.free(d_dst)
    return want


def test_encode_is_bit_identical_and_decodes_back():
    named = encode_sets()
    want = check_encode(named, "encode")
    by_name = dict(zip((n for n, _ in named), want))
    # the managed defect, byte for byte: 128 / 129 literals get the control bytes 0x80 / 0x81
    assert by_name["nonrepeating 128"] == b"\x80" + nonrepeating(128) and by_name["nonrepeating 129"] == b"\x81" + nonrepeating(129)
    assert by_name["nonrepeating 127"] == b"\xff" + nonrepeating(127)
    assert by_name["nonrepeating 130"] == b"\xff" + nonrepeating(127) + b"\x83" + nonrepeating(130)[127:]
    assert by_name["run 128"] == b"\x7fq\x81q" and by_name["run 130"] == b"\x7fq\x03q" and by_name["run 2"] == b"\x82qq" and by_name["0"] == b""
    defect = [W.rlhudson_has_defect(d) for _, d in named]
    assert [n for (n, _), bad in zip(named, defect) if bad and n.startswith("nonrepeating")] == ["nonrepeating 128", "nonrepeating 129"]
    # everything without the defect decodes back through the GPU decoder
    back = [item(w, len(d), name="back: " + n, want=(d, W.OK, len(d), len(w))) for (n, d), w, bad in zip(named, want, defect) if not bad]
    assert len(back) >= 200
    check_decode(back, "round trip")
    # ... and a stream with the defect does not
    bad = item(by_name["nonrepeating 129"], 129, name="the defect")
    assert bad["want"][1] != W.OK or bad["want"][0] != nonrepeating(129)
    check_decode([bad], "defect")


def test_encode_capacity_one_short():
    named = [(n, d) for n, d in encode_sets()[:60] if d]
    check_encode(named, "encode, one byte short", short=True)


def test_encode_bound_and_refusals():
    lib = ctx().lib
    for n in (0, 1, 2, 3, 127, 128, 1000):
        assert lib.alz_rlhudson_encode_bound(n) == W.rlhudson_encode_bound(n)
    worst = b"ab" * 500                                                # literals only: 1 control byte per 127
    assert len(W.rlhudson_encode(worst)) <= W.rlhudson_encode_bound(len(worst))
    # RLHudson is no fourth alz_rlh_format
    from auroralib.compression_amd import formats as F
    with pytest.raises(F.AlzError) as e:
        ctx().rlh_decode_batch((A.Stream * 1)(A.Stream(0, 0, 4, 16, 4, 0, 0, 3)), np.zeros(64, dtype=np.uint8), 64)
    assert e.value.code == A.E_INVALID and A.RLH_COUNT == 3
    # `format`, aux0 and aux1 are ignored
    s = (A.Stream * 1)(A.Stream(0, 0, 2, 5, 5, 0xFFFF, 0xFFFF, 77))
    dst, res = ctx().rlhudson_decode_batch(s, np.frombuffer(run(5, 0x61) + bytes(64), dtype=np.uint8), 5 + 64)
    assert (res[0].status, res[0].dst_len, res[0].src_used) == (0, 5, 2) and dst[:5].tobytes() == b"aaaaa"
