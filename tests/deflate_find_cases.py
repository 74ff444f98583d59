"""The inputs of tests/test_deflate_find_cpu.py and tests/test_gpu_deflate_find.py: per mechanism of alz_deflate_find_kernel the smallest
stream at which it can fail, and with each the tokens that PROVE the stream reaches it.  A case is dict(name, data, checks); a check is
(levels, position, kind, length, distance) with kind "match" (the token that starts at `position`), "lit" (a literal starts there) or
"covered" (no token starts there: an earlier match covers it).  The CPU test asserts every check on the restatement's tokens, so a case
that no longer reaches its mechanism fails there and not silently on the GPU.

Payloads are drawn from the byte values 200..255 and have no trigram twice; the background is noise over the 64 values 16..79 -- no
payload trigram occurs in it, and six bits a byte make a dynamic block smaller than the stored one, so the TOKENS of every case with a
check are in the stream's bytes (the CPU test asserts that no such block is stored) -- and a copy is fenced by two different bytes
(1, 2, ...) where its length matters.  lane = position mod 64 in every block (a block is 511 whole steps)."""
import heapq
import itertools
import random

import deflate_find_ref as R

B = R.BLOCK
ALL = tuple(range(1, 10))
GREEDY, LAZY = (1, 2, 3), (4, 5, 6, 7, 8, 9)
DEEP = ALL[1:]              # level 1 walks four candidates: in 32 KiB of noise a bucket holds two positions on average, and they stand in front
LENGTHS = (0, 1, 2, 3, 4) + tuple(range(62, 68)) + tuple(range(126, 132)) + tuple(range(257, 262))


def noise(n, seed):
    rng = random.Random(seed)
    return bytearray(16 + rng.randrange(64) for _ in range(n))


def pay(n, seed):
    """n bytes of 200..255: all different up to 56 of them, no trigram twice beyond"""
    rng = random.Random(1000 + seed)
    if n <= 56:
        return bytes(rng.sample(range(200, 256), n))
    out, seen = bytearray(rng.sample(range(200, 256), 2)), set()
    while len(out) < n:
        b = 200 + rng.randrange(56)
        t = bytes(out[-2:]) + bytes([b])
        if t in seen or b == out[-1]:
            continue
        seen.add(t)
        out.append(b)
    return bytes(out)


def put(buf, at, s):
    assert 0 <= at and at + len(s) <= len(buf)
    buf[at:at + len(s)] = s


def colliding_trigrams():
    """two different payload trigrams of one hash bucket, by the kernel's own hash"""
    seen = {}
    for t in itertools.permutations(range(200, 256), 3):
        h = R.trigram_hash(t[0] | (t[1] << 8) | (t[2] << 16))
        if h in seen and seen[h][0] != t[0]:
            return bytes(seen[h]), bytes(t)
        seen.setdefault(h, t)
    raise AssertionError("no collision")


def case(name, data, checks=()):
    return dict(name=name, data=bytes(data), checks=list(checks))


def synthetic():
    out = []
    # ---- lengths: a period of 7, so the one match runs to the stream's end
    seven = pay(7, 1)
    for n in LENGTHS:
        checks = [(ALL, 7, "match", n - 7, 7), (ALL, 6, "lit", 0, 0)] if n >= 10 else [(ALL, p, "lit", 0, 0) for p in range(n)]
        out.append(case("length %d" % n, (seven * 40)[:n], checks))

    # ---- links to a lane of the same step, and across steps
    d = noise(300, 2) + b"\xd0" * 700 + noise(5, 3)
    out.append(case("run", d, [(ALL, 300, "lit", 0, 0), (ALL, 301, "match", 258, 1), (ALL, 559, "match", 258, 1), (ALL, 817, "match", 183, 1)]))
    for P in (2, 3, 5, 63, 64, 65):
        d = noise(300, 10 + P) + (pay(P, P) * 400)[:700] + noise(5, 4)
        out.append(case("period %d" % P, d, [(ALL, 300 + P - 1, "lit", 0, 0), (ALL, 300 + P, "match", 258, P), (ALL, 558 + P, "match", 258, P)]))

    # ---- two different trigrams in one bucket.  A = triA + 37 bytes at 324 (step 5 = 320..383), its copy at 500
    tri_a, tri_b = colliding_trigrams()
    a_string = tri_a + pay(37, 20)
    for name, extra, checks in (
            ("same step, the colliding one later", [(370, tri_b)], [(ALL, 500, "lit", 0, 0), (ALL, 501, "match", 39, 176)]),
            ("same step, a third lane repeats the first", [(366, tri_b), (372, tri_a + b"\x03")], [(ALL, 500, "match", 40, 176)]),
            ("different steps", [(390, tri_b)], [(ALL, 500, "match", 40, 176)])):
        d = noise(600, 21)
        put(d, 324, a_string + b"\x01")
        for at, s in extra:
            put(d, at, s)
        put(d, 500, a_string + b"\x02")
        out.append(case("collision: " + name, d, checks))

    # ---- the skip carry
    s40 = pay(40, 30)
    for end in (511, 512, 513):
        d = noise(600, 31)
        put(d, 310, s40 + b"\x01")
        put(d, end - 40, s40 + b"\x02")
        out.append(case("a match that ends at %d" % end, d, [(ALL, end - 40, "match", 40, end - 350), (ALL, end - 1, "covered", 0, 0), (ALL, end, "lit", 0, 0)] +
                        ([(ALL, 512, "covered", 0, 0)] if end == 513 else [])))
    s258 = pay(258, 32)
    for lane in (0, 1, 62, 63):
        d = noise(1000, 33)
        put(d, 300, s258 + b"\x01")
        P = 640 + lane
        put(d, P, s258 + b"\x02")
        edges = [(ALL, e, "covered", 0, 0) for e in range(704, P + 258, 64) if e > P]
        out.append(case("258 bytes from lane %d" % lane, d, [(ALL, P, "match", 258, P - 300), (ALL, P + 257, "covered", 0, 0), (ALL, P + 258, "lit", 0, 0)] + edges))
    s516 = pay(516, 34)
    d = noise(1500, 35)
    put(d, 300, s516 + b"\x01")
    put(d, 900, s516 + b"\x02")
    out.append(case("258 back to back", d, [(ALL, 900, "match", 258, 600), (ALL, 1158, "match", 258, 600), (ALL, 1416, "lit", 0, 0)]))

    # ---- the lazy rule: "pqrs" matches 4 bytes at P, "qrstuvwxyz" 10 bytes at P + 1
    w = pay(11, 40)
    for lane in (0, 61, 62, 63):
        d = noise(600, 41)
        put(d, 310, w[:4] + b"\x01")
        put(d, 330, b"\x02" + w[1:] + b"\x03")
        P = 448 + lane
        put(d, P, w + b"\x04")
        greedy = [(P, "match", 4, P - 310), (P + 4, "match", 7, P + 4 - 334)]
        lazy = [(P, "lit", 0, 0), (P + 1, "match", 10, P + 1 - 331)]
        checks = [(GREEDY, *c) for c in greedy] + [(LAZY, *c) for c in (greedy if lane == 63 else lazy)]     # no look from lane 63 into the next step
        out.append(case("a longer match one byte on, lane %d" % lane, d, checks))

    # ---- three bytes at the distances around 4 096
    xyz = pay(3, 50)
    for dist in (4095, 4096, 4097):
        d = noise(300 + dist + 10, 51)
        put(d, 300, xyz + b"\x01")
        put(d, 300 + dist, xyz + b"\x02")
        out.append(case("three bytes at distance %d" % dist, d, [(ALL, 300 + dist, "match", 3, dist) if dist <= 4096 else (ALL, 300 + dist, "lit", 0, 0)]))

    # ---- the window
    for dist in (32767, 32768, 32769):
        d = noise(100 + dist + 650, 60)                   # (long enough behind the copy for the second block not to be stored)
        put(d, 100, s40 + b"\x01")
        put(d, 100 + dist, s40 + b"\x02")
        P = 100 + dist
        out.append(case("the only source at distance %d" % dist, d,
                        [(ALL, P, "match", 40, dist)] if dist <= 32768 else [(ALL, P, "lit", 0, 0), (ALL, P + 1, "lit", 0, 0), (ALL, P + 37, "lit", 0, 0)]))
    # the far edge: position 32778 (lane 10 of the step at 32 768) meets the 4 bytes at 54 first; the slot of 54 in prev holds the link of
    # 54 + 32 768 by then, so the 40 bytes at 10 -- 32 768 back, the true next candidate -- are never reached
    d = noise(32778 + 50, 61)
    put(d, 10, s40 + b"\x01")
    put(d, 54, s40[:4] + b"\x02")
    put(d, 32778, s40 + b"\x03")
    out.append(case("the far edge", d, [(DEEP, 32778, "match", 4, 32724), (DEEP, 32782, "match", 36, 32768)]))

    # ---- block edges.  Three blocks: a run across the first edge; the third block's history starts at 2 * 32704 - 32768 = 32640, where
    # 40 bytes lie whose copy opens the third block; a copy across the second edge
    d = noise(2 * B + 1000, 70)
    put(d, 32690, b"\xd0" * 600)
    put(d, 32640, s40 + b"\x01")
    put(d, 2 * B, s40 + b"\x02")
    put(d, 2 * B + 100, d[2 * B - 300:2 * B])
    out.append(case("three blocks", d, [(ALL, 32690, "lit", 0, 0), (ALL, 32691, "match", 13, 1), (ALL, B, "match", 258, 1), (ALL, B + 258, "match", 258, 1),
                                        (ALL, B + 516, "match", 70, 1), (ALL, 2 * B, "match", 40, 32768), (ALL, 2 * B + 100, "match", 258, 400),
                                        (ALL, 2 * B + 358, "match", 42, 400)]))
    # two blocks: a match cut by the block's end, its rest opening the next block; sources in the previous block at every distance class
    s320 = pay(320, 71)
    classes = (400, 4096, 4097, 20000, 32000, 32768)
    for r in (258, 3, 2, 1):
        d = noise(B + 400, 272 + r)
        put(d, B - r - 2000, s320 + b"\x01")
        put(d, B - r, s320[:r + 50] + b"\x02")
        checks = [(ALL, B - r, "match", r, 2000)] if r >= 3 else [(ALL, B - k, "lit", 0, 0) for k in range(r, 0, -1)]
        checks.append((ALL, B, "match", 50, 2000))
        for i, dist in enumerate(classes):
            q, s = B + 60 + 16 * i, pay(12, 80 + i)
            put(d, q - dist, s + b"\x01")
            put(d, q, s + b"\x02")
            checks.append((ALL if dist < 20000 else DEEP, q, "match", 12, dist))
        out.append(case("a match cut to %d by the block's end" % r, d, checks))

    # ---- the chain budget: `decoys` nearer positions with the same three bytes stand in front of the only long match
    g = pay(33, 90)
    for chain in sorted(set(R.level_chain(l) for l in ALL)):
        for decoys in (chain - 1, chain):
            d = noise(300, 91) + g + b"\x01" + b"".join(g[:3] + bytes([5 + i // 190, 5 + i % 190]) for i in range(decoys)) + b"\x04" + g + b"\x02" + noise(10, 92)
            P, near = 335 + 5 * decoys, 6
            checks = []
            for l in ALL:
                if decoys < R.level_chain(l):
                    checks.append(((l,), P, "match", 33, P - 300))
                elif R.level_lazy(l):
                    checks += [((l,), P, "lit", 0, 0), ((l,), P + 1, "match", 32, P - 300)]
                else:
                    checks.append(((l,), P, "match", 3, near))
            out.append(case("%d candidates in front of the long one" % decoys, d, checks))
    # ---- nice: a candidate of exactly `nice` bytes stands in front of one 20 bytes longer
    for nice in (32, 64, 128):
        h = pay(nice + 20, 95)
        d = noise(300, 96) + h + b"\x01" + noise(30, 97) + h[:nice] + b"\x02" + noise(30, 98) + h + b"\x03" + noise(10, 99)
        far, near, P = 300, 300 + nice + 51, 300 + 2 * nice + 82
        checks = []
        for l in ALL:
            if R.level_nice(l) > nice:
                checks.append(((l,), P, "match", nice + 20, P - far))
            elif not R.level_lazy(l):
                checks.append(((l,), P, "match", nice, P - near))
            else:                                  # P + 1 meets nice - 1 bytes first, walks on, finds the longer one: P becomes a literal
                checks += [((l,), P, "lit", 0, 0), ((l,), P + 1, "match", nice + 19, P - far)]
        out.append(case("nice %d" % nice, d, checks))

    # ---- plan edges
    out.append(case("one literal", b"\xd0"))
    out.append(case("one literal twice", b"\xd0\xd0"))
    out.append(case("no match at all", no_trigram_twice()))
    out.append(case("one distance symbol", b"r" * 600))
    out.append(case("stored ties with fixed", stored_fixed_tie()))
    out.append(case("fixed ties with dynamic", fixed_dynamic_tie()))
    out.append(case("the 15-bit cut", fibonacci_distances()))
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


TIE_LEVEL = 9


def _first_block(data, level=TIE_LEVEL):
    tokens = R.find(data, 0, level)
    lit_freq, dist_freq = R.histograms(tokens)
    return R.plan(lit_freq, dist_freq, len(data), len(tokens), True, False, False)


def stored_fixed_tie():
    """bytes above 143 take 9 bits in the fixed code: from 23 to 30 of them, all different, the fixed form is as long as the stored one"""
    for n in range(1, 57):
        data = pay(n, 110)
        p = _first_block(data)
        if R.block_bytes_of(p["size"][1], True) == 5 + n:
            return data
    raise AssertionError("no tie")


def fixed_dynamic_tie():
    """a prefix of word text whose fixed and dynamic forms take the same bytes, both below the stored one (at level TIE_LEVEL)"""
    import test_inflate_cpu as IC
    text = IC.text_like(700, 111)
    for n in range(40, 700):
        p = _first_block(text[:n])
        if R.block_bytes_of(p["size"][1], True) == R.block_bytes_of(p["size"][2], True) < 5 + n:
            return text[:n]
    raise AssertionError("no tie")


def no_trigram_twice():
    """66 bytes over four values in which each of the 64 trigrams stands once (a de Bruijn sequence, opened): no match exists, and two bits
    a byte make the block dynamic -- a dynamic header with an empty distance set"""
    k, n, a, seq = 4, 3, [0] * 12, []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(b"acgt"[v] for v in seq + seq[:2])


FIB_SYMBOLS = tuple(range(13, 30))
FIB_LEVELS = tuple(range(3, 10))


def fibonacci_distances():
    """Two blocks.  The first is 32 704 random bytes, a dictionary of four-byte slots.  The second is 4 180 copies of slots, each used once,
    back to back, at distances chosen so that the distance symbols 13 .. 29 occur 1, 1, 2, 3, 5, ... 1 597 times: the unlimited Huffman tree
    over these counts is 16 deep.  Near symbols come first (their sources are the end of the first block).  The counts are exact where the
    walk reaches every slot: a bucket of the 16 Ki holds two to four of the window's positions, so from level 3 on (16 candidates)."""
    rng = random.Random(120)
    d = bytearray(rng.randrange(256) for _ in range(B))
    free = [True] * (B // 4)
    counts, a, b = [], 1, 1
    for _ in FIB_SYMBOLS:
        counts.append(a)
        a, b = b, a + b
    tri = [d[q] | (d[q + 1] << 8) | (d[q + 2] << 16) for q in range(B - 2)]
    bucket = [R.trigram_hash(t) for t in tri]

    def on_a_chain(q):
        """no later lane of q's step holds another trigram of q's bucket (the collision bypass would take q off every chain)"""
        return all(bucket[r] != bucket[q] or tri[r] == tri[q] for r in range(q + 1, min((q | 63) + 1, B - 2)))
    last = None                                    # the byte behind the slot copied last: the next copy must not continue that match
    for s, c in zip(FIB_SYMBOLS, counts):
        e = (s >> 1) - 1
        base = 1 + ((2 + (s & 1)) << e)
        for _ in range(c):
            p = len(d)
            hi, lo = min(p - base, B - 4), max(p - (base + (1 << e) - 1), 0)
            slot = next(q for q in range((lo + 3) // 4, hi // 4 + 1) if free[q] and d[4 * q] != last and on_a_chain(4 * q))   # the farthest: it leaves the range first
            free[slot] = False
            last = d[4 * slot + 4] if 4 * slot + 4 < B else None
            d += d[4 * slot:4 * slot + 4]
    return bytes(d)


def unlimited_depth(freq):
    """the depth of a Huffman tree over the counts that are not 0, with no limit"""
    heap = [(f, 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        (f1, d1), (f2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1))
    return heap[0][1] if heap else 0


def load_test_bmp():
    """Test.bmp as tests/conftest.py's fixture recovers it (for tests/golden/make_deflate_find_vectors.py)"""
    import os
    import oracle_lib as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out, st = O.container_decompress(O.A.C_LZSS, open(os.path.join(root, "tests", "golden", "Test.lz"), "rb").read(), lz=O.A.LzProperties.from_bits(10, 6, 2))
    assert st == 0
    return out


def corpus(test_bmp):
    import test_inflate_cpu as IC
    return [case("Test.bmp at 54", test_bmp[54:54 + 70000]), case("Test.bmp at 600000", test_bmp[600000:670000]), case("word text", IC.text_like(70000, 7))]


def vectors(cases, stream_of=None):
    """"case|level|flags" -> [bytes, SHA-256] of the restatement's stream: what tests/golden/deflate_find_vectors.json holds.
    stream_of(case, level, flags): the stream where the caller has it already."""
    import hashlib
    out = {}
    for c in cases:
        for level in range(10):
            found = {}
            for flags in (0, R.FIXED_FLAG):
                s = stream_of(c, level, flags) if stream_of else b"".join(
                    b["bytes"] for b in R.blocks(c["data"], level, flags, tokens_of=lambda k: found.setdefault(k, R.find(c["data"], k, level))))
                out["%s|%d|%d" % (c["name"], level, flags)] = [len(s), hashlib.sha256(s).hexdigest()]
    return out


def token_map(blocks):
    """position -> the token that starts there, over the blocks of deflate_find_ref.blocks(); stored blocks show none"""
    at = {}
    for b in blocks:
        pos = b["start"]
        for t in b["tokens"]:
            at[pos] = t
            pos += 1 if t[0] == "lit" else t[1]
    return at


def failed_checks(c, level, blocks, data=None):
    """the checks of case `c` that the tokens of `blocks` (level `level`) do not meet"""
    at, bad = token_map(blocks), []
    for b in blocks:                               # (positions are counted from the tokens: they must add up to the block, or every check behind lies)
        covered = sum(1 if t[0] == "lit" else t[1] for t in b["tokens"])
        if covered != min(len(c["data"]) - b["start"], B):
            bad.append((c["name"], level, b["start"], "the tokens cover %d bytes of the block" % covered, 0, 0, None))
    for levels, pos, kind, length, dist in c["checks"]:
        if level not in levels:
            continue
        t = at.get(pos)
        ok = (t is None) if kind == "covered" else (t is not None and t[0] == "lit") if kind == "lit" else (t is not None and tuple(t[:3]) == ("match", length, dist))
        if not ok:
            bad.append((c["name"], level, pos, kind, length, dist, t))
    return bad
