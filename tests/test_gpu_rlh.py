"""-m gpu: the RLE30 / HUF20 family (alz_rlh_*) on the device, both kernel families, every result field and every output byte against the
pure-Python restatement (tests/rlh_ref.py) and, where one exists, the hand-assembled known answer (tests/golden/rlh_kat.json)."""
import random

import numpy as np
import pytest

import rlh_ref as R
import test_rlh_cpu as RC
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from cases import prose_like
from gpu_common import ctx

pytestmark = pytest.mark.gpu
FAMILIES = ((1, "exact"), (0, "production"))


# ---------------------------------------------------------------------------------------------- helpers
def pack(items, guard=0):
    """items: dicts(fmt, src, decom_len, cap, aux0) -> (streams, src array, dst_bytes); stream i sits at residue i mod 16 on both sides when
    `guard` is set, with `guard` untouched bytes around every destination"""
    n = len(items)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, guard
    for i, it in enumerate(items):
        b = bytes(it["src"])
        cap = it.get("cap", it["decom_len"])
        mis = (i % 16) if guard else 0
        chunks.append(bytes(mis) + b + bytes((-(len(b) + mis)) % 16))
        do += mis
        streams[i] = A.Stream(so + mis, do, len(b), cap, it["decom_len"], it.get("aux0", 0), 0, it["fmt"])
        so += len(chunks[-1])
        do = (do + cap + guard + 15) // 16 * 16
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 64


def expect(items):
    """the restatement's answer per item, computed once"""
    for it in items:
        if "want" not in it:
            it["want"] = R.decode(it["fmt"], it["src"], it["decom_len"], it.get("cap", it["decom_len"]), it.get("aux0", 0))
    return items


def check_decode(items, what):
    expect(items)
    streams, src, dst_bytes = pack(items)
    for exact, fam in FAMILIES:
        ctx().set_exact_kernels(exact)
        try:
            dst, res = ctx().rlh_decode_batch(streams, src, dst_bytes)
        finally:
            ctx().set_exact_kernels(0)
        for i, it in enumerate(items):
            out, status, dst_len, src_used = it["want"]
            tag = "%s [%s] stream %d (%s)" % (what, fam, i, it.get("name", A.RLH_NAMES[it["fmt"]]))
            print("%s: gpu status=%d len=%d used=%d | ref status=%d len=%d used=%s" % (tag, res[i].status, res[i].dst_len, res[i].src_used, status, dst_len, src_used))
            assert (res[i].status, res[i].dst_len) == (status, dst_len), tag
            if src_used is not None:
                assert res[i].src_used == src_used, tag
            a = streams[i].dst_off
            got = dst[a:a + dst_len].tobytes()
            if got != out:
                d = next(k for k in range(dst_len) if got[k] != out[k])
                raise AssertionError("%s: byte %d of %d differs (gpu %d, ref %d)" % (tag, d, dst_len, got[d], out[d]))


def run(n, b):
    return bytes([0x80 | (n - 3), b])


def lit(data):
    return bytes([len(data) - 1]) + bytes(data)


def rle_item(src, size, cap=None, name=""):
    return dict(fmt=A.RLH_RLE30, src=src, decom_len=size, cap=size if cap is None else cap, name=name)


def random_tokens(rng, nbytes):
    """a valid RLE30 stream of random elements and what it decodes to"""
    s, out = bytearray(), bytearray()
    while len(out) < nbytes:
        if rng.random() < 0.5:
            n, b = rng.choice([3, 4, 5, 17, 64, 65, 129, 130]), rng.randrange(256)
            s += run(n, b); out += bytes([b]) * n
        else:
            d = bytes(rng.randrange(256) for _ in range(rng.choice([1, 1, 2, 3, 7, 63, 64, 65, 127, 128])))
            s += lit(d); out += d
    return bytes(s), bytes(out)


# ---------------------------------------------------------------------------------------------- known answers
def test_all_kats():
    items = []
    for c in RC.kats():
        want = (bytes.fromhex(c["out"]), c["status"], c["dst_len"], c["src_used"])
        it = dict(fmt=c["fmt"], src=bytes.fromhex(c["src"]), decom_len=c["decom_len"], cap=c["cap"], aux0=c["aux0"], name=c["name"])
        ref = R.decode(it["fmt"], it["src"], it["decom_len"], it["cap"], it["aux0"])
        assert ref[:3] == want[:3] and (want[3] is None or ref[3] == want[3]), c["name"]
        it["want"] = want
        items.append(it)
    check_decode(items, "kat")


# ---------------------------------------------------------------------------------------------- RLE30 decode
def rle30_shape_items():
    rng = random.Random(30)
    items = []
    pad = lit(bytes(range(100))) * 8                                  # 808 input bytes in front: the lane-parallel rounds need > 588 bytes ahead
    for ntok in (63, 64, 65):                                          # element counts around one round's 64
        for kind in ("run3", "lit1", "mixed"):
            toks = [(run(3, 0x10 + k) if kind == "run3" or (kind == "mixed" and k & 1) else lit(bytes([k]))) for k in range(ntok)]
            tail = lit(bytes(range(90))) * 8                           # ... and behind, so that these elements are not the exact tail's
            s = b"".join(toks) + tail
            size = len(R.rle30_decode(s, 1 << 20, 1 << 20)[0])
            items.append(rle_item(s, size, name="%d x %s" % (ntok, kind)))
    for size in (1023, 1024, 1025):                                    # output sizes around the 1 KiB a 64-lane pass of 16-byte granules writes
        body = lit(bytes(range(127))) + run(130, 7) * 6 + lit(bytes(range(116)))      # 127 + 780 + 116 = 1023
        s = body + {1023: b"", 1024: lit(b"z"), 1025: lit(b"zy")}[size] + pad
        items.append(rle_item(s, size, name="%d bytes" % size))
        items.append(rle_item(pad + s, 800 + size, name="800 + %d bytes" % size))
    items.append(rle_item(run(130, 0xEE) * 300, 39000, name="all runs of 130"))
    items.append(rle_item(b"".join(lit(bytes([k & 0xFF])) for k in range(2500)), 2500, name="all literals of 1"))
    items.append(rle_item(b"".join(lit(bytes((k + j) & 0xFF for j in range(128))) + run(3, k & 0xFF) for k in range(150)), 150 * 131, name="128 literals / run of 3"))
    for k in range(5):
        s, out = random_tokens(rng, rng.choice([700, 3000, 6000, 12000]))
        items.append(rle_item(s, len(out), name="random elements %d" % k))
        items.append(rle_item(s, len(out) - rng.randrange(1, 200), cap=len(out), name="random elements %d, declared short" % k))   # the last element overshoots or is never read
    prose = prose_like(65536, 31)
    zeros = bytearray(65536)
    for k in range(0, 65536, 997):
        zeros[k] = 1 + k % 255
    for name, data in (("prose", prose), ("mostly zero", bytes(zeros))):
        s = R.rle30_encode(data)
        items.append(rle_item(s, len(data), name="64 KiB " + name))
    total = sum(it["cap"] for it in items)
    assert total < 300 << 10, total
    return items


def test_rle30_decode_shapes():
    check_decode(rle30_shape_items(), "rle30 shapes")


# ---------------------------------------------------------------------------------------------- RLE30 encode
def encode_sets():
    sets = [("empty", b""), ("1", b"a"), ("2", b"ab"), ("3", b"abc"), ("3 equal", b"aaa")]
    sets += [("nonrepeating %d" % n, RC.nonrepeating(n)) for n in (126, 127, 128, 129, 130, 131, 254, 255, 256, 257, 1000)]
    sets += [("run %d" % n, b"q" * n) for n in (2, 3, 4, 126, 127, 128, 129, 130, 254, 255, 1000)]
    sets += [("ab + run + de", b"ab" + b"c" * 300 + b"de"), ("pairs", b"aabbccddee" * 40), ("triples", b"aaabbbcccdddeee" * 40),
             ("prose", prose_like(20000, 41)), ("zeros", bytes(9000)), ("shape data", rle30_shape_items()[-1]["src"][:4000])]
    return sets


def check_encode(named, what, caps=None):
    n = len(named)
    streams = (A.Stream * n)()
    chunks, so, do = [], 0, 0
    for i, (_, d) in enumerate(named):
        cap = caps[i] if caps else R.rle30_encode_bound(len(d)) + 8
        streams[i] = A.Stream(so, do, len(d), cap, 0, 0, 0, A.RLH_RLE30)
        chunks.append(d + bytes((-len(d)) % 16))
        so += len(chunks[-1]); do += (cap + 15) // 16 * 16
    src = np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy()
    want = [R.rle30_encode(d) for _, d in named]
    for fam in ("one kernel for both families",):                      # (alz_ctx_set_exact_kernels does not change the encoder: nothing to run twice)
        dst, res = ctx().rlh_encode_batch(streams, src, do + 64)
        for i, (name, d) in enumerate(named):
            tag = "%s [%s] %s (%d bytes)" % (what, fam, name, len(d))
            if len(want[i]) > streams[i].dst_cap:
                assert (res[i].status, res[i].dst_len) == (A.ST_OUTPUT_CAPACITY, 0), tag
                continue
            assert (res[i].status, res[i].dst_len, res[i].src_used) == (A.ST_OK, len(want[i]), len(d)), tag
            a = streams[i].dst_off
            assert dst[a:a + len(want[i])].tobytes() == want[i], tag


def test_rle30_encode_is_bit_identical():
    check_encode(encode_sets(), "rle30 encode")


def test_rle30_encode_ragged_batch_and_capacity():
    rng = np.random.default_rng(64)
    named = []
    for k in range(64):
        n = int(rng.integers(0, 3000))
        d = bytearray(prose_like(n, 100 + k))
        for _ in range(int(rng.integers(0, 6))):                       # some runs of every length class
            a, ln = int(rng.integers(0, max(n, 1))), int(rng.integers(2, 400))
            d[a:a + ln] = bytes([int(rng.integers(0, 256))]) * len(d[a:a + ln])
        named.append(("ragged %d" % k, bytes(d)))
    check_encode(named, "rle30 ragged batch")
    sizes = [len(R.rle30_encode(d)) for _, d in named]
    check_encode(named, "rle30 capacity", caps=[max(0, s + (k % 3) - 1) for k, s in enumerate(sizes)])   # one below, at, one above the need
    # the decoder reads what the encoder wrote (the defect aside: these end in a run)
    d = prose_like(5000, 9) + b"\0" * 40
    comp = R.rle30_encode(d)
    check_decode([rle_item(comp, len(d), name="round trip")], "rle30 round trip")


# ---------------------------------------------------------------------------------------------- HUF20 decode
def huf_item(stream, size, bits, big=False, cap=None, name=""):
    return dict(fmt=A.RLH_HUF20_4 if bits == 4 else A.RLH_HUF20_8, src=stream, decom_len=size, cap=size if cap is None else cap, aux0=1 if big else 0, name=name)


def test_huf20_decode_data_sets():
    items = []
    for name, data, depths in RC.huf_sets():
        for bits in depths:
            for big in ((False, True) if bits == 4 else (False,)):
                s = R.huf20_build(data, bits, big)
                assert s is not None, name
                items.append(huf_item(s, len(data), bits, big, name="%s %d-bit%s" % (name, bits, " big" if big else "")))
                if name == "fixed3":
                    # fixed-length codes never self-synchronise: the worst case of the speculative rounds.  Sizes that end mid-round and mid-word.
                    for size in (4095, 4033, 2731, 1366, 683, 342, 171, 64, 11, 1):
                        items.append(huf_item(s, size, bits, big, name="%s, %d bytes of it%s" % (name, size, " big" if big else "")))
    assert sum(it["cap"] for it in items) < 300 << 10
    check_decode(items, "huf20 sets")


def test_huf20_codes_longer_than_a_word():
    """A chain tree of 34 nodes (tests/golden/make_kats_rlh.py: codes of 1 to 34 bits).  The words behind the one that holds the last symbol are
    not read, although a lane-parallel round has them in hand: src_used must stop where the managed Position stops, for every declared size --
    also the sizes at which a round of 64 words ends exactly on the last symbol, or in the middle of a long code."""
    tree = bytearray([34, 0x80])
    for j in range(33):
        tree += bytes([0x30 + j, 0x80 if j < 32 else 0xC0])
    tree += bytes([0x61, 0x62])
    code = {0x30 + j: "1" * j + "0" for j in range(33)}
    code[0x61], code[0x62] = "1" * 33 + "0", "1" * 33 + "1"

    def stream(syms):
        bits = "".join(code[v] for v in syms)
        bits += "0" * (-len(bits) % 32)
        return bytes(tree) + b"".join(int(bits[k:k + 32], 2).to_bytes(4, "little") for k in range(0, len(bits), 32))
    rng = random.Random(34)
    items = []
    # the reviewer's shape: 62 words of one-bit codes, then the front of a 34-bit code in words 63 / 64
    s = stream([0x30] * 1984 + [0x61])
    assert len(s) == 70 + 256
    for size in (1983, 1984, 1985):
        items.append(huf_item(s, size, 8, name="62 words of '0', declared %d" % size))
    # mixed lengths over several rounds, every declared size in steps that hit round ends and code middles
    syms = [rng.choice([0x30] * 12 + [0x31, 0x32, 0x35, 0x3F, 0x4F, 0x50, 0x61, 0x62]) for _ in range(2600)]
    s = stream(syms) + bytes(8)
    assert len(s) > 70 + 3 * 256
    for size in list(range(1, len(syms), 41)) + [len(syms) - 1, len(syms), len(syms) + 1]:
        items.append(huf_item(s, size, 8, name="mixed code lengths, declared %d" % size))
    nib = bytearray(tree)
    for k in range(2, len(nib)):
        if k % 2 == 0 or k == len(nib) - 1:
            nib[k] &= 0x0F                                           # (leaf values as nibbles for the 4-bit mode; node bytes stay)
    for size in (700, 992, 993, 1300):
        items.append(huf_item(bytes(nib) + s[70:], size, 4, big=bool(size & 1), name="4-bit, declared %d" % size))
    check_decode(items, "huf20 long codes")


# ---------------------------------------------------------------------------------------------- malformed input
def valid_streams():
    base = prose_like(3000, 77) + bytes(300) + prose_like(700, 78)
    return {A.RLH_RLE30: (R.rle30_encode(base), len(base)), A.RLH_HUF20_8: (R.huf20_build(base, 8), len(base)), A.RLH_HUF20_4: (R.huf20_build(base, 4), len(base))}


@pytest.mark.parametrize("fmt", range(A.RLH_COUNT), ids=A.RLH_NAMES)
def test_every_prefix_length_class(fmt):
    comp, size = valid_streams()[fmt]
    cuts = sorted(set([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 33, 130, 131, 513, 514, 515, 516, 517, 518, 600, 1100, len(comp) // 3, len(comp) // 2,
                       len(comp) - 5, len(comp) - 4, len(comp) - 3, len(comp) - 2, len(comp) - 1, len(comp)]))
    check_decode([dict(fmt=fmt, src=comp[:c], decom_len=size, cap=size, name="prefix %d of %d" % (c, len(comp))) for c in cuts], "prefixes")


def fuzz_items(fmt, seed=1234, count=96):
    """the four kinds of tests/cases.py::fuzz_items: noise, bit flips, splices, biased noise"""
    rng = random.Random(seed + fmt)
    comp, size = valid_streams()[fmt]
    items = []
    for k in range(count):
        kind = k % 4
        if kind == 0:
            n = rng.choice([0, 1, 2, 7, 63, 64, 129, 587, 588, 589, 1000, 1500, 4000, 9000])
            src = bytes(rng.randrange(256) for _ in range(n))
            if fmt != A.RLH_RLE30 and n >= 2 and rng.random() < 0.5:
                src = bytes([rng.choice([1, 2, 3, 8, 31])]) + src[1:]      # small trees: more streams that get past the first bits
        elif kind == 1:
            b = bytearray(comp)
            for _ in range(rng.randrange(1, 6)):
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            src = bytes(b)
        elif kind == 2:
            cut = rng.randrange(len(comp))
            src = comp[:cut] + bytes(rng.randrange(256) for _ in range(rng.randrange(1, 3000))) + comp[cut:]
        else:
            n = rng.randrange(1100, 6000)
            src = bytes(rng.choice([0, 0, 0xFF, 0x0F, 0xF0, 0x80, 0xC0, rng.randrange(256)]) for _ in range(n))
        decl = rng.choice([0, 1, 50, 400, size])
        cap = rng.choice([decl, decl + 300, max(decl, 1) // 2, decl - 1 if decl else 0])
        items.append(dict(fmt=fmt, src=src, decom_len=decl, cap=cap, aux0=k & 1 if fmt == A.RLH_HUF20_4 else 0, name="fuzz kind %d" % kind))
    return items


@pytest.mark.parametrize("fmt", range(A.RLH_COUNT), ids=A.RLH_NAMES)
def test_fuzz(fmt):
    items = expect(fuzz_items(fmt))
    seen = {it["want"][1] for it in items}
    print("statuses seen:", sorted(seen))
    assert {R.OK, R.INPUT_TRUNCATED, R.OUTPUT_CAPACITY} <= seen           # the noise reaches every kind of ending
    if fmt != A.RLH_RLE30:
        assert any(it["want"][1] == R.INPUT_TRUNCATED and it["want"][3] not in (None, len(it["src"])) for it in items)   # an index beyond the tree
    check_decode(items, "fuzz")


def test_capacities_below_at_and_above():
    items = []
    for fmt, (comp, size) in valid_streams().items():
        for decl, cap in [(size, size), (size, size + 300), (size, size - 1), (size, size // 2), (size, 0), (size - 10, size - 10), (size - 10, size + 10),
                          (size // 2, size // 2), (size // 2, size // 2 + 1), (1, 1), (0, 0), (size + 500, size + 500)]:
            items.append(dict(fmt=fmt, src=comp, decom_len=decl, cap=cap, name="declared %d into %d" % (decl, cap)))
    check_decode(items, "capacities")


def test_api_refusals():
    s = (A.Stream * 1)(A.Stream(0, 0, 4, 16, A.HUF20_MAX_DECOM, 0, 0, A.RLH_HUF20_8))
    src = np.zeros(64, dtype=np.uint8)
    for fn, st in ((ctx().rlh_decode_batch, s), (ctx().rlh_encode_batch, (A.Stream * 1)(A.Stream(0, 0, 4, 16, 0, 0, 0, A.RLH_HUF20_4))),
                   (ctx().rlh_encode_batch, (A.Stream * 1)(A.Stream(0, 0, 4, 16, 0, 0, 0, A.RLH_HUF20_8)))):
        with pytest.raises(F.AlzError) as e:
            fn(st, src, 64)
        assert e.value.code == A.E_UNSUPPORTED
    with pytest.raises(F.AlzError) as e:
        ctx().rlh_decode_batch((A.Stream * 1)(A.Stream(0, 0, 4, 16, 4, 0, 0, A.RLH_COUNT)), src, 64)
    assert e.value.code == A.E_INVALID


# ---------------------------------------------------------------------------------------------- canary: device-resident, every residue mod 16
def test_canary_device_resident():
    items = []
    for fmt, (comp, size) in valid_streams().items():
        items += [dict(fmt=fmt, src=comp, decom_len=size, cap=size), dict(fmt=fmt, src=comp, decom_len=size, cap=size - 7), dict(fmt=fmt, src=comp[:len(comp) // 2], decom_len=size, cap=size),
                  dict(fmt=fmt, src=comp, decom_len=size - 33, cap=size + 40), dict(fmt=fmt, src=comp, decom_len=1001, cap=1001), dict(fmt=fmt, src=comp, decom_len=65, cap=64)]
        items += fuzz_items(fmt, seed=99, count=16)
    for k, it in enumerate(rle30_shape_items()[:24]):
        items.append(it)
    for c in RC.kats():
        items.append(dict(fmt=c["fmt"], src=bytes.fromhex(c["src"]), decom_len=c["decom_len"], cap=c["cap"], aux0=c["aux0"], name=c["name"]))
    assert len(items) >= 96                                            # every residue mod 16 several times, on both sides
    expect(items)
    GUARD = 48
    streams, src, dst_bytes = pack(items, guard=GUARD)
    c = ctx()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes)
    try:
        c.h2d(d_src, src)
        for exact, fam in FAMILIES:
            c.memset(d_dst, 0xA5, dst_bytes)
            c.set_exact_kernels(exact)
            try:
                res = c.rlh_decode_batch_device(streams, d_src, src.nbytes - 64, d_dst, dst_bytes - 64)
            finally:
                c.set_exact_kernels(0)
            assert c.last_kernel_ms() > 0
            dst = c.d2h(d_dst, dst_bytes)
            touched = np.zeros(dst_bytes, dtype=bool)
            for i, it in enumerate(items):
                out, status, dst_len, src_used = it["want"]
                tag = "canary [%s] stream %d (%s)" % (fam, i, it.get("name", A.RLH_NAMES[it["fmt"]]))
                assert (res[i].status, res[i].dst_len) == (status, dst_len), tag
                if src_used is not None:
                    assert res[i].src_used == src_used, tag
                a = streams[i].dst_off
                assert dst[a:a + dst_len].tobytes() == out, tag
                # RLE30 writes its dst_len bytes and nothing else; a HUF20 stream that failed may have written inside min(dst_cap, decom_len)
                w = dst_len if it["fmt"] == A.RLH_RLE30 or status == R.OK else min(streams[i].dst_cap, it["decom_len"])
                touched[a:a + w] = True
            bad = np.nonzero(~touched & (dst != 0xA5))[0]
            assert bad.size == 0, "canary [%s]: %d guard bytes changed, first at %d" % (fam, bad.size, bad[0])
        # the encoder: nothing outside [dst_off, dst_off + dst_len), also when dst_cap is one short
        named = [("enc %d" % k, prose_like(200 + 37 * k, k) + bytes(k)) for k in range(32)]
        want = [R.rle30_encode(d) for _, d in named]
        e_items = [dict(fmt=A.RLH_RLE30, src=d, decom_len=0, cap=len(w) - (k % 2)) for k, ((_, d), w) in enumerate(zip(named, want))]
        e_streams, e_src, e_dst_bytes = pack(e_items, guard=GUARD)
        d_es, d_ed = c.malloc(e_src.nbytes), c.malloc(e_dst_bytes)
        try:
            c.h2d(d_es, e_src)
            c.memset(d_ed, 0xA5, e_dst_bytes)
            res = c.rlh_encode_batch_device(e_streams, d_es, e_src.nbytes - 64, d_ed, e_dst_bytes - 64)
            dst = c.d2h(d_ed, e_dst_bytes)
            touched = np.zeros(e_dst_bytes, dtype=bool)
            for k, w in enumerate(want):
                a = e_streams[k].dst_off
                if k % 2:
                    assert (res[k].status, res[k].dst_len) == (A.ST_OUTPUT_CAPACITY, 0), k
                    touched[a:a + e_streams[k].dst_cap] = True             # (what a failed encode left inside its capacity is unspecified)
                else:
                    assert (res[k].status, res[k].dst_len) == (A.ST_OK, len(w)) and dst[a:a + len(w)].tobytes() == w, k
                    touched[a:a + len(w)] = True
            assert not np.any(~touched & (dst != 0xA5))
        finally:
            c.free(d_es); c.free(d_ed)
    finally:
        c.free(d_src); c.free(d_dst)


# ---------------------------------------------------------------------------------------------- containers
def test_containers():
    data = prose_like(9000, 55) + bytes(500) + prose_like(800, 56) + b"\0\0\0\0"
    body = R.rle30_encode(data)
    rle, lz77, l5 = F.RLE30(), F.LZ77(), F.Level5()
    lz77.Type, l5.Type = F.LZ77.RLE30, F.Level5.RLE
    files = {"RLE30": (rle, R.gba_header(0x30, len(data)) + body), "LZ77": (lz77, b"LZ77" + R.gba_header(0x30, len(data)) + body),
             "Level5": (l5, (4 | len(data) << 3).to_bytes(4, "little") + body)}
    for name, (obj, want) in files.items():
        comp = obj.Compress(data)
        assert comp == want, name                                      # header + the restatement's body
        assert obj.Decompress(comp) == data and obj.GetDecompressedSize(comp) == len(data), name
        assert obj.last_src_used == len(comp), name
        if name != "Level5":
            assert obj.IsMatch(comp), name
    assert F.Level5().Compress(data, F.CompressionSettings.Fastest)[:4] == (len(data) << 3).to_bytes(4, "little")     # quality 0 -> OnlySave (Level5.cs:120-121)
    l5h = F.Level5()
    l5h.Type = F.Level5.Huffman4Bit
    assert l5h.Compress(data, F.CompressionSettings.Fastest)[4:] == data      # ... also in front of the Huffman refusal
    # the defect travels through the container: 129 non-repeating bytes compress to a stream that does not decode back
    comp = rle.Compress(RC.nonrepeating(129))
    assert comp == b"\x30\x81\x00\x00\x80" + RC.nonrepeating(129)
    assert R.rle30_decode(comp[4:], 129, 129 + 273)[1] == R.INPUT_TRUNCATED          # (0x80 reads as a run of 3; the literals then read as controls)
    with pytest.raises(F.EndOfStreamException):
        rle.Decompress(comp)
    with pytest.raises(F.EndOfStreamException):
        rle.Decompress(files["RLE30"][1][:-3])
    # HUF20 files are assembled by the test builder (there is no encoder)
    huf = F.HUF20()
    for bits, t in ((4, 0x24), (8, 0x28)):
        f = R.gba_header(t, len(data)) + R.huf20_build(data, bits, big=False)
        assert huf.IsMatch(f) and huf.GetDecompressedSize(f) == len(data) and huf.Decompress(f) == data and huf.last_src_used == len(f)
        assert F.LZ77().Decompress(b"LZ77" + f) == data and F.LZ77().IsMatch(b"LZ77" + f)
        g = ((2 if bits == 4 else 3) | len(data) << 3).to_bytes(4, "little") + R.huf20_build(data, bits, big=True)     # Level5: Endian.Big
        assert F.Level5().Decompress(g) == data
        with pytest.raises(F.EndOfStreamException):
            huf.Decompress(f[:-4])
        with pytest.raises(BufferError):
            huf.Decompress(f, capacity=len(data) - 1)
    big = R.gba_header(0x28, 0x1000000) + R.huf20_build(b"ab", 8)
    assert huf.GetDecompressedSize(big) == 0x1000000
    # the dispatch around the new types is untouched: an LZ10 file and a ChunkLZ10 file still decode
    chunked = F.LZ77()
    chunked.Type, chunked.ChunkSize = F.LZ77.ChunkLZ10, 0x800
    assert chunked.Decompress(chunked.Compress(data)) == data
    assert F.LZ77().Decompress(F.LZ77().Compress(data)) == data and F.LZ10().Decompress(F.LZ10().Compress(data)) == data
    assert F.Level5().Decompress(F.Level5().Compress(data)) == data
