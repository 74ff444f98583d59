"""Hand-built LZ4 frames / legacy files / Snappy framed streams for the container tests."""
import random
import struct


def lz4_len_ext(n):
    out = bytearray()
    n -= 15
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def lz4_linked_blocks(seed, nblocks, block_bytes, max_dist=65535):
    """Random LZ4 blocks whose matches reach back across block boundaries (one window per frame, LZ4.Frame.cs:120).
    Returns (list of compressed blocks, expected output), the output computed by a plain byte-wise model."""
    rng = random.Random(seed)
    out = bytearray()
    blocks = []
    for _ in range(nblocks):
        blk = bytearray()
        start = len(out)
        while len(out) - start < block_bytes:
            lit = bytes(rng.randrange(256) for _ in range(min(int(rng.expovariate(1 / 6.0)), 300)))
            if not out and not lit:
                lit = b"x"
            mlen = 4 + min(int(rng.expovariate(1 / 10.0)), 600)
            dist = rng.randint(1, min(len(out) + len(lit), max_dist))
            if rng.random() < 0.1:
                dist = min(dist, rng.randint(1, 4))
            tok = (min(len(lit), 15) << 4) | min(mlen - 4, 15)
            blk.append(tok)
            if len(lit) >= 15:
                blk += lz4_len_ext(len(lit))
            blk += lit
            out += lit
            blk += struct.pack("<H", dist)
            if mlen - 4 >= 15:
                blk += lz4_len_ext(mlen - 4)
            for _ in range(mlen):
                out.append(out[-dist])
        lit = bytes(rng.randrange(256) for _ in range(5 + rng.randrange(20)))     # last sequence: literals only
        blk.append(min(len(lit), 15) << 4)
        if len(lit) >= 15:
            blk += lz4_len_ext(len(lit))
        blk += lit
        out += lit
        blocks.append(bytes(blk))
    return blocks, bytes(out)


def lz4_frame(blocks, xxh32, flg=0x40, bd=0x40, content=None, raw_flags=None, content_size=None):
    """Frame around ready-made blocks.  flg bits: 4 content checksum, 8 content size, 16 block checksum, 32 independent."""
    desc = bytearray([flg, bd])
    if flg & 8:
        desc += struct.pack("<Q", content_size if content_size is not None else len(content))
    hc = (xxh32(bytes(desc)) >> 8) & 0xFF
    f = bytearray(struct.pack("<I", 0x184D2204)) + desc + bytes([hc])
    for i, b in enumerate(blocks):
        raw = bool(raw_flags and raw_flags[i])
        f += struct.pack("<I", len(b) | (0x80000000 if raw else 0)) + b
        if flg & 16:
            f += struct.pack("<I", xxh32(b))
    f += struct.pack("<I", 0)
    if flg & 4:
        f += struct.pack("<I", xxh32(content))
    return bytes(f)


def lz4_legacy(blocks, eof_flag=True):
    f = bytearray(struct.pack("<I", 0x184C2102))
    for b in blocks:
        f += struct.pack("<I", len(b)) + b
    if eof_flag:
        f.append(0xFF)
    return bytes(f)


# ------------------------------------------------------------------------------------------------ generated files + mutations
# Framed files with their expected output from a byte-wise model of the managed readers (one window per LZ4 frame, offset 0 = distance
# 65 536 (E1), zeros in front of a window's start (E2), a fresh window per legacy block and per Snappy chunk), and a seeded mutator that
# works on the structure the generator recorded.  The generator and the mutator do not call the C oracle: checksum functions are passed in.
import os  # noqa: E402

SEED = int(os.environ.get("ALZ_FUZZ_SEED", "1234"))


class Model:
    """The output of a file so far; `origin` is where the current window starts (bytes in front of it read as zeros)."""

    def __init__(self):
        self.out = bytearray()
        self.origin = 0

    def lit(self, b):
        self.out += b

    def match(self, dist, n):
        d = dist or 65536                                                  # E1
        start = len(self.out) - d
        k = min(d, n)
        first = bytearray(k)                                               # E2: zeros in front of the window's start
        lo = max(start, self.origin)
        if lo < start + k:
            first[lo - start:] = self.out[lo:start + k]
        self.out += (bytes(first) * (n // k + 1))[:n]                      # (a match longer than its distance repeats with that period)


class File:
    """Bytes plus the fields they are made of: (kind, offset, length, info) -- what the mutator changes."""

    def __init__(self):
        self.b = bytearray()
        self.fields = []

    def put(self, kind, data, info=None):
        self.fields.append((kind, len(self.b), len(data), info))
        self.b += data


def lz4_seq(lit, dist=None, mlen=0):
    """One LZ4 sequence: literals, then (unless dist is None) a match of mlen >= 4 bytes at distance dist (0 = 65 536)."""
    ml = mlen - 4 if dist is not None else 0
    b = bytearray([(min(len(lit), 15) << 4) | min(ml, 15)])
    if len(lit) >= 15:
        b += lz4_len_ext(len(lit))
    b += lit
    if dist is not None:
        b += struct.pack("<H", dist)
        if ml >= 15:
            b += lz4_len_ext(ml)
    return bytes(b)


def lz4_block(rng, m, n, kind="random", reach="block"):
    """Compressed bytes of one LZ4 block that adds exactly n bytes to the model.  kind: random | maxratio | literals | zero (starts with an
    offset-0 match) | empty (the one-byte block 0x00).  reach: block (matches stay in the block), frame (anywhere in the window), before
    (also in front of the window's start)."""
    start = len(m.out)
    blk = bytearray()
    if kind == "empty":
        return b"\x00"
    if kind == "literals":
        lit = rng.randbytes(n)
        m.lit(lit)
        return lz4_seq(lit)
    if kind == "maxratio":                                                 # one length-extension byte after another: about 255 : 1
        k = min(rng.randint(1, 8), n)
        lit = rng.randbytes(k if n - k >= 4 else n)
        m.lit(lit)
        if n - k < 4:
            return lz4_seq(lit)
        m.match(k, n - k)
        return lz4_seq(lit, k, n - k)
    if kind == "zero":
        lit = rng.randbytes(rng.choice((0, 0, 3)))
        mlen = min(rng.randint(4, 40), max(n - len(lit), 0))
        if mlen >= 4:
            m.lit(lit)
            m.match(0, mlen)
            blk += lz4_seq(lit, 0, mlen)
    while len(m.out) - start < n:
        left = n - (len(m.out) - start)
        base = {"block": start, "frame": m.origin, "before": -(1 << 40)}[reach]
        lit = rng.randbytes(min(max(int(rng.expovariate(1 / 8.0)), 1 if len(m.out) <= base else 0), 300, left))
        avail = min(len(m.out) + len(lit) - base, 65535)
        mlen = min(4 + min(int(rng.expovariate(1 / 24.0)), 3000), left - len(lit))
        if mlen < 4 or avail < 1:
            lit = rng.randbytes(left)
            m.lit(lit)
            blk += lz4_seq(lit)
            break
        dist = rng.randint(1, avail)
        if rng.random() < 0.15:
            dist = min(dist, rng.randint(1, 4))
        m.lit(lit)
        m.match(dist, mlen)
        blk += lz4_seq(lit, dist, mlen)
    return bytes(blk)


BMAX = {4: 0x10000, 5: 0x40000, 6: 0x100000, 7: 0x400000}


def lz4_frame_into(f, m, rng, xxh32, bd, blocks, flg=0x40, content_size_delta=0):
    """Appends one frame to File f.  blocks: (kind, n, reach) with kind as lz4_block's, or 'stored' (raw, high bit) / 'stored1'."""
    m.origin = frame_start = len(m.out)
    f.put("magic", struct.pack("<I", 0x184D2204))
    bmax = BMAX[bd]
    body = []
    for kind, n, reach in blocks:
        o = len(m.out)
        if kind in ("stored", "stored1"):
            raw = rng.randbytes(n)
            m.lit(raw)
            body.append((raw, True, o))
        else:
            body.append((lz4_block(rng, m, n, kind, reach), False, o))
    content = bytes(m.out[frame_start:])
    desc = bytearray([flg, bd << 4])
    f.put("flg", bytes(desc))
    if flg & 8:
        f.put("csize", struct.pack("<Q", len(content) + content_size_delta))
    f.put("hc", bytes([(xxh32(bytes(desc) + (struct.pack("<Q", len(content) + content_size_delta) if flg & 8 else b"")) >> 8) & 0xFF]))
    mids = []
    for b, raw, o in body:
        assert len(b) <= bmax, (len(b), bmax)
        f.put("size", struct.pack("<I", len(b) | (0x80000000 if raw else 0)), bmax)
        f.put("body", b)
        if flg & 16:
            f.put("bsum", struct.pack("<I", xxh32(b)))
        mids.append(o)
    f.put("end", struct.pack("<I", 0))
    if flg & 4:
        f.put("csum", struct.pack("<I", xxh32(content)))
    return mids


def lz4_legacy_into(f, m, rng, blocks, eof_flag=True):
    """Appends a legacy file (a fresh window per block): blocks as (kind, n)."""
    f.put("magic", struct.pack("<I", 0x184C2102))
    mids = []
    for kind, n in blocks:
        m.origin = o = len(m.out)
        b = lz4_block(rng, m, n, kind, "before")
        f.put("lsize", struct.pack("<I", len(b)))
        f.put("body", b)
        mids.append(o)
    if eof_flag:
        f.put("eof", b"\xff")
    return mids


def _snappy_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def snappy_body(rng, m, n, zeros=False):
    """A Snappy raw body (varint size, then literal / copy-1 / copy-2 / copy-4 elements) adding exactly n bytes; a fresh window."""
    m.origin = start = len(m.out)
    b = bytearray(_snappy_varint(n))
    while len(m.out) - start < n:
        left = n - (len(m.out) - start)
        have = len(m.out) - start
        if zeros and have == 0:
            lit = bytes(1)
        elif zeros or (have and rng.random() < 0.6):
            lit = None
        else:
            lit = rng.randbytes(min(1 + int(rng.expovariate(1 / 20.0)), 70000 if rng.random() < 0.05 else 300, left))
        if lit is not None:
            L = len(lit) - 1
            if L < 60:
                b.append(L << 2)
            else:
                k = (L.bit_length() + 7) // 8
                b.append((59 + k) << 2)
                b += L.to_bytes(k, "little")
            b += lit
            m.lit(lit)
            continue
        kind = rng.choice((1, 2, 2, 3)) if not zeros else 2
        dist = 1 if zeros else rng.randint(1, min(have, 65535) if rng.random() > 0.03 else 65535)   # (rarely in front of the chunk: zeros)
        if kind == 1 and dist < 2048 and left >= 4:
            ln = rng.randint(4, min(11, left))
            b += bytes([1 | ((ln - 4) << 2) | ((dist >> 8) << 5), dist & 0xFF])
        elif kind == 3:
            ln = rng.randint(1, min(64, left))
            b += bytes([3 | ((ln - 1) << 2)]) + struct.pack("<I", dist)
        else:
            ln = rng.randint(1, min(64, left))
            b += bytes([2 | ((ln - 1) << 2)]) + struct.pack("<H", dist)
        m.match(dist, ln)
    return bytes(b)


def crc32c_py(data):
    c = 0xFFFFFFFF
    for x in data:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 & -(c & 1))
    return c ^ 0xFFFFFFFF


def snappy_file(rng, m, chunks):
    """chunks: ('c', n) compressed, ('z', n) compressed zeros, ('s', n) stored, ('S', n) stored zeros, ('k', n) skippable."""
    f = File()
    f.put("magic", bytes([0xff, 0x06, 0x00, 0x00]) + b"sNaPpY")
    mids = []
    for kind, n in chunks:
        o = len(m.out)
        if kind in "cz":
            body = snappy_body(rng, m, n, zeros=kind == "z")
            typ, payload = 0, body
        elif kind in "sS":
            payload = bytes(n) if kind == "S" else rng.randbytes(n)
            m.lit(payload)
            typ = 1
        else:
            typ, payload = rng.randint(0x80, 0xFE), rng.randbytes(n)
        crc = b"" if typ >= 0x80 else struct.pack("<I", 0)          # (checksums are not verified: Snappy.cs skips them)
        ln = len(payload) + len(crc)
        f.put("chunk", bytes([typ, ln & 0xFF, (ln >> 8) & 0xFF, ln >> 16]), typ)
        if crc:
            f.put("crc", crc)
        if typ == 0:
            v = _snappy_varint(n)
            f.put("varint", v)
            f.put("body", payload[len(v):])
        else:
            f.put("body", payload)
        if typ < 0x80:
            mids.append(o)
    return f, mids


class Case:
    """One generated file: container ('lz4' | 'legacy' | 'snappy'), bytes, expected output (None for a mutant), block starts in the output."""

    def __init__(self, label, container, f, expect, mids, seed, fields=None):
        self.label, self.container, self.seed = label, container, seed
        self.data = bytes(f.b) if isinstance(f, File) else bytes(f)
        self.fields = f.fields if isinstance(f, File) else (fields or [])
        self.expect = None if expect is None else bytes(expect)
        self.mids = mids

    def __repr__(self):
        return "%s[seed %d]" % (self.label, self.seed)


def _frame_case(label, seed, xxh32, bd, blocks, flg=0x40):
    rng, m, f = random.Random(seed), Model(), File()
    mids = lz4_frame_into(f, m, rng, xxh32, bd, blocks, flg)
    return Case(label, "lz4", f, m.out, mids, seed)


def generated_cases(xxh32, seed=SEED):
    """The valid shapes (SEED: ALZ_FUZZ_SEED).  Every case carries the model's output."""
    s = seed * 1000
    K = 1024
    cases = []
    # block sizes: full, short in the middle, short last, one byte long -- BD 4/5/6/7
    for i, bd in enumerate((4, 5, 6, 7)):
        bm = BMAX[bd]
        full = "maxratio" if bd >= 6 else "random"
        cases.append(_frame_case("bd%d full+short-mid+short-last" % bd, s + i, xxh32, bd,
                                 [(full, bm, "block"), ("random", 3000, "block"), (full, bm, "block"), ("random", 777, "block")]))
        cases.append(_frame_case("bd%d one-byte blocks" % bd, s + 10 + i, xxh32, bd,
                                 [("random", 5000, "block"), ("empty", 0, "block"), ("stored1", 1, "block"), ("random", 900, "block"), ("stored1", 1, "block")]))
    # stored blocks first, in the middle, last (full stored blocks: what does not compress)
    cases.append(_frame_case("bd4 stored first/mid/last", s + 20, xxh32, 4,
                             [("stored", 0x10000, ""), ("random", 0x10000, "block"), ("stored", 0x10000, ""), ("literals", 20000, ""), ("stored", 4000, "")], flg=0x40 | 16 | 4))
    cases.append(_frame_case("bd5 stored mid, independent", s + 21, xxh32, 5,
                             [("random", 0x40000, "block"), ("stored", 0x40000, ""), ("random", 0x40000, "block")], flg=0x60 | 8))
    # compression ratio: beyond 32 : 1 up to the maximum, at 64 KiB, 1 MiB, 4 MiB; next to stored and short blocks
    cases.append(_frame_case("bd4 max-ratio 64K", s + 30, xxh32, 4, [("maxratio", 0x10000, ""), ("maxratio", 0x10000, ""), ("random", 0x10000, "block")]))
    cases.append(_frame_case("bd6 max-ratio 1M + stored + short", s + 31, xxh32, 6,
                             [("maxratio", 0x100000, ""), ("stored", 50000, ""), ("maxratio", 0x100000, ""), ("random", 2000, "block")], flg=0x40 | 16))
    cases.append(_frame_case("bd7 max-ratio 4M + short (split plans)", s + 32, xxh32, 7,
                             [("maxratio", 0x400000, ""), ("maxratio", 0x400000, ""), ("random", 3000, "block")]))
    cases.append(_frame_case("bd7 40:1 blocks + short", s + 33, xxh32, 7,
                             [("random", 0x400000, "block"), ("maxratio", 0x300000, ""), ("random", 20000, "block")]))
    cases.append(_frame_case("bd4 block larger than its maximum", s + 34, xxh32, 4,
                             [("random", 0x10000, "block"), ("maxratio", 0x18000, ""), ("random", 0x10000, "block")]))
    # linked frames: across blocks, in front of the frame's start (after an earlier frame: zeros, not its bytes), flags both ways
    for j, flg in enumerate((0x40, 0x60, 0x40 | 4 | 8 | 16, 0x60 | 16)):
        cases.append(_frame_case("bd4 linked flg=%02x" % flg, s + 40 + j, xxh32, 4,
                                 [("random", 30000, "frame"), ("random", 0x10000, "frame"), ("stored", 2000, ""), ("random", 20000, "frame"), ("empty", 0, "")], flg=flg))
    rng, m, f = random.Random(s + 45), Model(), File()
    mids = lz4_frame_into(f, m, rng, xxh32, 4, [("random", 40000, "block")])
    mids += lz4_frame_into(f, m, rng, xxh32, 5, [("random", 30000, "before"), ("random", 50000, "before")], flg=0x40 | 4)
    cases.append(Case("linked, in front of the second frame's start", "lz4", f, m.out, mids, s + 45))
    cases.append(_frame_case("bd5 linked far", s + 46, xxh32, 5, [("random", 0x40000, "frame"), ("random", 0x40000, "frame"), ("random", 5000, "frame")], flg=0x40 | 16))
    # offset 0 (distance 65 536) at history below, at and above 65 536, and inside a block
    for j, hist in enumerate((1000, 0x10000, 100000)):
        bd = 4 if hist <= 0x10000 else 5
        first = [("stored", hist, "")] if hist <= BMAX[bd] else [("random", hist, "block")]
        cases.append(_frame_case("offset 0 at history %d" % hist, s + 50 + j, xxh32, bd, first + [("zero", 3000, "frame"), ("random", 2000, "frame")]))
    cases.append(_frame_case("offset 0 inside a block", s + 53, xxh32, 5, [("random", 0x11000, "block"), ("zero", 0x12000, "block")]))
    # flags: content size, content checksum, block checksums present and absent, independence set and clear
    for j, flg in enumerate((0x40 | 8, 0x40 | 4, 0x40 | 16, 0x60 | 4 | 8 | 16, 0x60)):
        cases.append(_frame_case("bd4 flags %02x" % flg, s + 60 + j, xxh32, 4, [("random", 0x10000, "block"), ("random", 0x10000, "block"), ("random", 1234, "block")], flg=flg))
    # concatenation: frame + skippable + legacy + frame, trailing junk
    rng, m, f = random.Random(s + 70), Model(), File()
    mids = lz4_frame_into(f, m, rng, xxh32, 4, [("random", 20000, "frame"), ("random", 9000, "frame")])
    f.put("skip", struct.pack("<II", 0x184D2A5A, 7) + rng.randbytes(7))
    mids += lz4_legacy_into(f, m, rng, [("random", 30000), ("random", 100)], eof_flag=False)
    mids += lz4_frame_into(f, m, rng, xxh32, 5, [("random", 40000, "before")], flg=0x40 | 4)
    f.put("junk", b"\x01\x02\x03\x04junk")
    cases.append(Case("frame+skippable+legacy+frame+junk", "lz4", f, m.out, mids, s + 70))
    # legacy files: 8 MiB blocks (full, max ratio), short in the middle and last, one byte long, with and without the EOF flag
    for j, (blocks, eof) in enumerate((([("maxratio", 0x800000), ("random", 5000), ("maxratio", 0x800000), ("random", 300)], True),
                                       ([("random", 70000), ("empty", 0), ("literals", 1), ("zero", 0x11000)], False),
                                       ([("maxratio", 0x400000), ("random", 0x20000)], True))):
        rng, m, f = random.Random(s + 80 + j), Model(), File()
        mids = lz4_legacy_into(f, m, rng, blocks, eof_flag=eof)
        cases.append(Case("legacy %d" % j, "legacy", f, m.out, mids, s + 80 + j))
    # Snappy: stored, compressed and skippable chunks in every order, chunks of zeros, full 64 KiB chunks
    import itertools
    for j, order in enumerate(itertools.permutations("csk")):
        rng, m = random.Random(s + 90 + j), Model()
        chunks = [(k, {"c": rng.randint(1, 0x10000), "s": rng.randint(1, 3000), "k": rng.randint(0, 40)}[k]) for k in order]
        f, mids = snappy_file(rng, m, chunks + [("c", 0x10000)])
        cases.append(Case("snappy " + "".join(order), "snappy", f, m.out, mids, s + 90 + j))
    rng, m = random.Random(s + 99), Model()
    f, mids = snappy_file(rng, m, [("z", 0x10000), ("S", 5000), ("c", 0x10000), ("s", 0x10000), ("z", 3), ("k", 0), ("c", 1)])
    cases.append(Case("snappy zeros", "snappy", f, m.out, mids, s + 99))
    return cases


def many_tiny_blocks(xxh32, nblocks=20000):
    """A frame of 20 000 one-byte blocks at BD 7 (about 100 KB): the capacity hint used to ask for their block maximum each."""
    return _frame_case("bd7 %d one-byte blocks" % nblocks, 7, xxh32, 7, [("stored1", 1, "")] * nblocks)


def _with(data, off, new, old_len=None):
    return bytes(data[:off]) + bytes(new) + bytes(data[off + (len(new) if old_len is None else old_len):])


def mutants(case, seed, per_case=12):
    """Seeded structural mutations of a generated file: size fields +-1 / high bit / above the block maximum, truncation at field boundaries,
    byte flips inside a body, flipped block and content checksums, EndMark removed or doubled, content size off by one; for Snappy the chunk
    lengths, types and declared sizes.  Returns Cases without an expected output (the oracle decides)."""
    rng = random.Random(seed)
    d, out = case.data, []

    def add(what, data):
        out.append(Case("%s / %s" % (case.label, what), case.container, data, None, case.mids, case.seed))

    by = {}
    for fl in case.fields:
        by.setdefault(fl[0], []).append(fl)
    pick = lambda k: rng.choice(by[k]) if by.get(k) else None  # noqa: E731
    for kind in ("size", "lsize"):
        fl = pick(kind)
        if fl:
            _, o, _, bmax = fl
            v = struct.unpack("<I", d[o:o + 4])[0]
            for nv in (v + 1, v - 1, v ^ 0x80000000, (bmax or 0x800000) + 1):
                add("%s@%d %#x->%#x" % (kind, o, v, nv & 0xFFFFFFFF), _with(d, o, struct.pack("<I", nv & 0xFFFFFFFF)))
    bounds = sorted({fl[1] for fl in case.fields} | {fl[1] + fl[2] for fl in case.fields})
    for cut in rng.sample(bounds[1:], min(len(bounds) - 1, 5)):
        add("truncated at field boundary %d" % cut, d[:cut])
    bodies = [fl for fl in by.get("body", []) if fl[2]]
    for _ in range(3):
        if bodies:
            _, o, n, _ = rng.choice(bodies)
            p = o + rng.randrange(n)
            add("flip body byte %d" % p, _with(d, p, bytes([d[p] ^ (1 << rng.randrange(8))])))
    for kind in ("bsum", "csum"):
        fl = pick(kind)
        if fl:
            add("flip %s@%d" % (kind, fl[1]), _with(d, fl[1], bytes([d[fl[1]] ^ 0x10])))
    fl = pick("end")
    if fl:
        add("EndMark removed @%d" % fl[1], _with(d, fl[1], b"", 4))
        add("EndMark doubled @%d" % fl[1], _with(d, fl[1], bytes(8), 4))
    fl = pick("csize")
    if fl:
        v = struct.unpack("<Q", d[fl[1]:fl[1] + 8])[0]
        for nv in (v + 1, v - 1):
            add("content size %d->%d" % (v, nv), _with(d, fl[1], struct.pack("<Q", nv & (2 ** 64 - 1))))
    fl = pick("chunk")
    if fl:
        _, o, _, typ = fl
        ln = d[o + 1] | (d[o + 2] << 8) | (d[o + 3] << 16)
        for nl in (ln + 1, ln - 1, ln + 1000):
            nl &= 0xFFFFFF
            add("chunk length@%d %d->%d" % (o, ln, nl), _with(d, o + 1, bytes([nl & 0xFF, (nl >> 8) & 0xFF, nl >> 16])))
        add("chunk type@%d %#x->%#x" % (o, typ, typ ^ 1), _with(d, o, bytes([typ ^ 1])))
    fl = pick("varint")
    if fl:
        _, o, n, _ = fl
        v = 0
        for i in range(n):
            v |= (d[o + i] & 0x7F) << (7 * i)
        for nv in (v + 1, v - 1, 0):
            if nv >= 0:
                add("declared size@%d %d->%d" % (o, v, nv), _with(d, o, _snappy_varint(nv), n))
    rng.shuffle(out)
    return out[:per_case] if per_case else out


def snappy_refusal_reached(data, cap):
    """The documented deviation: the library refuses (E_FORMAT) a compressed chunk whose body does not end at its declared length; the
    oracle reads on from where the body stopped.  True when the oracle's in-order walk reaches such a chunk before any failure."""
    import oracle_lib as O
    from auroralib.compression_amd import _abi as A
    pos, out = 10, 0
    while pos < len(data):
        if pos + 4 > len(data):
            return False
        typ, cl = data[pos], int.from_bytes(data[pos + 1:pos + 4], "little")
        pos += 4
        if typ == 0:
            if pos + 4 > len(data):
                return False
            _, r = O.decode_stream(A.FMT_SNAPPY_RAW, data[pos + 4:], cap=max(cap - out, 0))
            if r.status != A.ST_OK:
                return False
            if r.src_used + 4 != cl:
                return True
            out += r.dst_len
            pos += 4 + r.src_used
        elif typ == 1:
            if pos + 4 > len(data) or cl < 4:
                return False
            n = min(cl - 4, len(data) - pos - 4)
            if out + n > cap:
                return False
            out += n
            pos += 4 + n
        elif typ <= 0x7F:
            return False
        else:
            pos = min(pos + cl, len(data))
    return False
