"""Built inputs for the search stage of the LZ encoder (csrc/alz_encode.hip: match_search_b with PRUNE and WAVEPOS, enc_match_kernel, enc_match_dyn_kernel,
enc_match_dense_kernel, enc_probe_kernel, the compare cap of choose_b_cap).  Pure Python; shared by tests/test_encode_search_cpu.py (every case proves itself
against the oracle and the finder restatement) and tests/test_gpu_encode_search.py (every encoder path on them).

A case is a raw buffer -- a background and ONE proving place -- and a claim: the chain at the proving position P (the earlier positions whose four bytes hash
like P's, nearest first, with the number of bytes each has in common with P) and the token the reference writes at P.  The kernels decide at numbers (a class of
8 lanes, a best length of 16, a cap of 48 or 256, exactly maxChain attempts); each case stands on one side of one of them, and the parse visits P, so a kernel
that answers differently there changes the compared bytes.

How a buffer is laid out
  background  random bytes of 0x20 .. 0xFF (`noise`).  Bytes below 0x20 are kept for the proving place and for the run of the lane variant, so no word of the
              background is a word of the case.  Groups of four background bytes may repeat by chance, and a background word may hash like the case's:
              `build` redraws the buffer until the chain at P is the stated one at every quality's hash width.
  candidates  in [P - 2000, P): strings that start with the case's word W (four bytes below 0x10) and go on like the target for a stated number of bytes,
              each ended by a byte that differs.  All of them and P share W, so they are one hash class at every hash width: the chain is known.
  target      at P, a multiple of 256 (and of 64): the kernels' ranges and wavefronts start there.  P = 8448, so every buffer is longer than 8 KiB (the
              whole-GPU path's threshold) whatever stands behind P.
  variants    `dense`: the buffer as built -- fewer than 1 / 8 of the probe's samples hit, the stream goes to the two-phase kernel; `lane`: a run of
              0x1E 0x1F a quarter longer than the buffer behind it (in front of it, a multiple of 256, where the case needs the stream's end) -- more than
              half of the samples hit, the stream goes to the one-position-per-lane kernel.  probe_counts restates the rule; the CPU file asserts the margins.

Rows and qualities: ROWS, QUALITIES below.  What a grammar, a geometry or a quality cannot express, and what this file leaves to other tests, is listed in
NOT_EXPRESSIBLE with the reason, per row and quality."""
import functools
import zlib

import numpy as np

import chain_finder_ref as CF
import geometry_cases as G
from auroralib.compression_amd import _abi as A

P0 = 8448                                            # the proving position: 33 * 256
QUALITIES = (1, 3, 8, 12)                            # maxChain 2 (lane kernel, PRUNE), 4 (dense, blocks of 64), 16 (dense DYN), 128 (the min-length table, enc_match_dyn_kernel)
# row of geometry_cases -> writer of token_bodies.EDGE_FORMATS
ROWS = {"yaz0": "yaz0", "lz10": "lz10", "lz11": "lz11", "lz4_block": "lz4_block", "lzss_12_4_2_compat": "lzss_12_4_2", "lz10_vram": "lz10", "refpack": "refpack",
        "snappy_raw": "snappy_raw"}
S_ONLY = ("snappy_raw",)                             # family S alone: the 32 KiB window and the links behind ALZ_SCAN_NEAR blocks of enc_scan_seq_kernel
FAMILIES = ("K1", "K2", "K3", "K4", "K5", "N", "S")
SCAN_QUALITIES = (3, 8, 9)                           # S: the scan path covers qualities 2 .. 9; 9 has maxChain 24 -- more than 16 candidates in one block
SCAN_Q10_ROWS = ("lz4_block", "snappy_raw")          # ... and quality 10 (maxChain 32) where min_len is 4: no min-length table there (use_min_table = q >= 10 && min_len < 4)
SCAN_ROWS = ("yaz0", "lz10", "lz11", "lz4_block", "lzss_12_4_2_compat", "lz10_vram", "snappy_raw")      # (test_gpu_scan_encode.FAM, one property set)
RUN = b"\x1e\x1f"
FRONT = b"\x1a"

NOT_EXPRESSIBLE = {}                                 # (row, quality, family, case) -> why

def _no(row, q, family, case, why):
    NOT_EXPRESSIBLE[(row.name, q, family, case)] = why


def tail_skip(row):
    return 5 if row.fmt == A.FMT_LZ4_BLOCK else 0       # the finder sees all but the last five bytes  LZ4.cs:208


@functools.lru_cache(maxsize=None)
def finder(name, q):
    """the restated finder of (row, quality): its numbers (max_chain, lazy, hash_bits, max_len, ...) and ScoreMatch"""
    row = G.BY_NAME[name]
    return CF.ChainFinder(row.finder_props(), q, **row.finder_kw())


def b_cap(row, q):
    """choose_b_cap (alz_encode.hip): the compare cap of kernel B in the regular pipeline, None where there is none"""
    f = finder(row.name, q)
    if f.max_len < 96:
        return None
    cap = 48 if f.max_chain <= 5 or f.max_chain >= 64 else 256
    return cap if f.max_len > cap else None


# ------------------------------------------------------------------------------------------------ restatements
def hashes(data, bits):
    """ComputeHash of every position that has four bytes  LzChainMatchFinder.cs:288-299"""
    a = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.uint64)
    n = len(a)
    if n < 4:
        return np.zeros(0, dtype=np.uint64)
    v = a[:n - 3] | (a[1:n - 2] << 8) | (a[2:n - 1] << 16) | (a[3:] << 24)
    return ((v * CF.PRIME) & CF.M32) >> (32 - bits)


def chain_at(data, p, bits):
    """the earlier positions with P's hash, nearest first: what head / chain hold when the cursor stands on P (every position up to `limit` is inserted, :134-144, :196-203)"""
    h = hashes(data, bits)
    return np.nonzero(h[:p] == h[p])[0][::-1].tolist()


def common(data, a, b, mx):
    n = 0
    while n < mx and data[a + n] == data[b + n]:
        n += 1
    return n


def pick(name, q, data, p):
    """MatchSearch without the min-length table (:214-225, ChainMatches :248-282) at ONE position, from the brute-force chain -> (distance, length)"""
    f = finder(name, q)
    n = len(data)
    best_possible = min(n - p, f.max_len)
    best_d = best_l = 0
    best_score, attempts = -1, f.max_chain
    for c in chain_at(data, p, f.hash_bits):
        if attempts <= 0:
            break
        attempts -= 1
        d = p - c
        if d > f.max_dist:
            break
        if d < f.min_dist:
            continue
        score, ln = f._score(common(data, p, c, best_possible), d)
        if score > best_score:
            best_score, best_l, best_d = score, ln, d
            if best_l == best_possible:
                break
    return best_d, best_l


def probe_counts(name, q, data):
    """enc_probe_kernel restated -> (hit, tot): the sampled positions (k * 64 + lane) * step, the first link at the finder's hash width, sixteen bytes equal.
    (Sixteen bytes at a position near the stream's end reach into the slack behind it: such a sample counts as no hit here and the margins absorb it.)"""
    row, f = G.BY_NAME[name], finder(name, q)
    n = len(data) - tail_skip(row)
    limit = n - 4
    if limit < 64:
        return 0, 0
    step = max((limit + 1) // 1024, 1)
    h = hashes(data[:n], f.hash_bits).tolist()
    last, prev = {}, [-1] * len(h)
    for i, v in enumerate(h):
        prev[i] = last.get(v, -1)
        last[v] = i
    hit = tot = 0
    for s in range(1024):
        pos = s * step
        if pos > limit:
            break
        tot += 1
        c = prev[pos]
        d = pos - c if c >= 0 else 0
        if d > 0 and f.min_dist <= d <= f.max_dist and d <= 0xFFFF and pos + 16 <= len(data) and data[pos:pos + 16] == data[c:c + 16]:
            hit += 1
    return hit, tot


def lane_side(hit, tot):
    """the probe's line: hit * 16 >= tot * ALZ_PROBE_THRESH16 (4)"""
    return hit * 16 >= tot * 4


# ------------------------------------------------------------------------------------------------ the builder
class Buf:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.b = bytearray()
        w = self.rng.permutation(15)[:4] + 1             # the case's word: four different bytes of 1 .. 15
        self.W = bytes(int(x) for x in w)
        self.enders = list(range(0x10, 0x1A))             # bytes that end a candidate: never in the background, never in W (0x1A stands in front of P, 0x1B ends the target, 0x1C / 0x1D are the decoy's)

    def noise(self, k):
        self.b += self.rng.integers(0x20, 0x100, k, dtype=np.uint8).tobytes()
        return self

    def to(self, pos):
        assert pos >= len(self.b), (pos, len(self.b))
        return self.noise(pos - len(self.b))

    def text(self, k):
        return self.rng.integers(0x20, 0x100, k, dtype=np.uint8).tobytes()


def colliders(W, k, seed):
    """k words of four bytes whose 15-bit hash is W's and whose 16-bit hash is not (so no wider hash of theirs is W's either): found by drawing"""
    rng = np.random.default_rng(seed)
    own = (int.from_bytes(W, "little") * CF.PRIME) & CF.M32
    out = []
    while len(out) < k:
        v = rng.integers(0x20, 0x100, (1 << 18, 4), dtype=np.uint64)      # (background bytes: a collider brings no reserved byte with it)
        w = v[:, 0] | (v[:, 1] << 8) | (v[:, 2] << 16) | (v[:, 3] << 24)
        h = (w * CF.PRIME) & CF.M32
        for x in w[((h >> 17) == (own >> 17)) & ((h >> 16) != (own >> 16))].tolist():
            out.append(int(x).to_bytes(4, "little"))
    return out[:k]


def place(seed, lens, target_len, gap=9, tail=200, dists=None, before=b"", decoy=False, W=None, P=P0, collide=0):
    """`lens`: bytes each candidate has in common with the target, NEAREST FIRST (each at least 4); the target has `target_len` bytes of its own and an ender,
    then `tail` background bytes (0: the stream ends with the target).  `dists`: explicit distances for some candidates {index: distance}.  `before`: bytes put
    directly in front of P.  decoy: a four-byte match for P - 1 (the byte in front of P and three bytes of W, planted early), so that P is the lazy neighbour.
    -> (data, P, [(position, common bytes)] nearest first)"""
    bf = Buf(seed)
    if W is not None:
        bf.W = W
    if not before and not decoy:
        before = FRONT                                   # (a background byte there could lengthen a candidate's match to the front: the cursor would not stand on P)
    longest = max([target_len] + list(lens)) + 8
    body = bf.text(longest)
    T = bf.W + body
    width = [max(ln, 4) + 1 + gap for ln in lens]
    P0 = P                                               # (N: the proving position at the range edges of enc_narrow_lds_kernel)
    at, cur = [], P0 - 24 - 8 * collide - len(before)
    for i, ln in enumerate(lens):                        # nearest first: from P backwards
        if dists and i in dists:
            cur = P0 - dists[i]
        else:
            cur -= width[i]
        at.append(cur)
    first = min(at) if at else P0
    assert first >= 64, first
    bf.noise(40)
    if decoy:
        assert first > P0 - 2900
        bf.to(P0 - 3000)                                 # (inside every row's window)
        z = 0x1D
        bf.b += bytes([z]) + bf.W[:3] + bytes([0x1C])
        before = bytes([z])
    order = sorted(range(len(lens)), key=lambda i: at[i])
    for i in order:
        bf.to(at[i])
        ln = lens[i]
        bf.b += T[:ln] + bytes([bf.enders[i % len(bf.enders)]])      # (ln > target_len: it goes on like what would stand BEHIND the target)
    bf.to(P0 - len(before))
    bf.b += before
    assert len(bf.b) == P0
    for i, w in enumerate(colliders(bf.W, collide, seed)):   # between the nearest candidate and P: on P's 15-bit chain, not on its chain at the finder's width
        bf.b[P0 - len(before) - 8 * (i + 1):P0 - len(before) - 8 * (i + 1) + 4] = w
    bf.b += T[:target_len]
    if tail:
        bf.b += bytes([0x1B])
        bf.noise(tail)
    return bytes(bf.b), P0, [(at[i], min(lens[i], target_len)) for i in range(len(lens))]


def copy_place(seed, d, a, total, cuts, tail=200, n_end=None):
    """K1: a source of `total` + a bytes and its copy at distance d, the copy starting at P - a; the copy's bytes at P + c, c in `cuts`, are replaced.  The
    positions of the wavefront [P, P + 64) whose four bytes hold no replaced byte have their first candidate at distance d.  n_end: the stream ends there."""
    bf = Buf(seed)
    src_at = P0 - a - d
    assert src_at >= 40
    bf.to(src_at)
    S = bf.text(total + a)
    bf.b += S
    if len(bf.b) > P0 - a:                               # d < len: the copy overlaps its source -- take the bytes as they come
        del bf.b[P0 - a:]
    bf.to(P0 - a)
    bf.b[-1:] = FRONT
    for i in range(total + a):
        bf.b.append(bf.b[len(bf.b) - d])
    for k, c in enumerate(cuts):
        bf.b[P0 + c] = 0x10 + k
    if n_end is not None:
        del bf.b[n_end:]
    elif tail:
        bf.b += bytes([0x1B])
        bf.noise(tail)
    return bytes(bf.b)


def variant(data, lane, end):
    """the lane variant: a run a quarter longer than the buffer, behind it -- in front of it (a multiple of 256 bytes) where the case needs the stream's end"""
    if not lane:
        return data, 0
    k = (len(data) * 5 // 4 + 255) // 256 * 256 + 256
    run = (RUN * (k // 2))
    return (run + data, k) if end else (data + run, 0)


class Case:
    def __init__(self, name, data, p, cands=None, end=False, start=False, claim=None):
        self.name, self.data, self.p, self.cands, self.end, self.start = name, data, p, cands, end, start
        self.claim = claim or {}

    def buffer(self, lane):
        """(data, P) of a variant"""
        d, shift = variant(self.data, lane, self.end)
        return d, self.p + shift


def lane_classes(data, base, bits):
    """{distance: lanes} over the wavefront [base, base + 64): the first candidate of every lane -- the nearest earlier position with the lane's hash --, as
    match_search_b's WAVEPOS branch sees it in its first trip (lanes behind `limit` and lanes without a candidate are left out)"""
    h = hashes(data, bits)
    out = {}
    for pos in range(base, min(base + 64, len(h))):
        at = np.flatnonzero(h[:pos] == h[pos])
        if len(at):
            out[pos - int(at[-1])] = out.get(pos - int(at[-1]), 0) + 1
    return out


def block_pairs(name, q, data, base, size):
    """the pairs enc_match_dense_kernel lists for the block [base, base + size): per position the candidates of its walk -- at most maxChain attempts, ended by a
    candidate beyond max_dist -- that are not nearer than min_dist"""
    f = finder(name, q)
    h = hashes(data, f.hash_bits)
    total = 0
    for pos in range(base, min(base + size, len(h))):
        at = np.flatnonzero(h[:pos] == h[pos])[::-1][:f.max_chain]
        for c in at.tolist():
            if pos - c > f.max_dist:
                break
            total += pos - c >= f.min_dist
    return total


def claim_holds(name, case, lane):
    """what a case states about its hash classes, re-derived from the buffer at every quality's hash width: the chain at P (or its first entry), the
    distance classes of the proving wavefront (`classes`: the lanes of each stated distance, exactly, and fewer than 8 lanes at any other distance -- a
    background word may hash like an earlier one --; `class_of`: the lanes of ONE distance),
    the pairs of the proving block at maxChain 4 (`pairs`) and of the block of 256 positions at maxChain 16 (`pairs_dyn`)"""
    row = G.BY_NAME[name]
    data, p = case.buffer(lane)
    data = data[:len(data) - tail_skip(row)]
    base = p - case.claim.get("lane", 0)
    for bits in sorted({finder(name, q).hash_bits for q in QUALITIES + (9, 10)}):
        got = chain_at(data, p, bits)
        if case.cands is not None and got != [p - case.p + c for c, _ in case.cands]:
            return False
        if case.cands is None and case.claim.get("first") is not None and (not got or p - got[0] != case.claim["first"]):
            return False
        if "classes" in case.claim:
            found = lane_classes(data, base, bits)
            if any(found.get(d, 0) != k for d, k in case.claim["classes"].items()) or any(k >= 8 for d, k in found.items() if d not in case.claim["classes"]):
                return False
        if "class_of" in case.claim:
            d, k = case.claim["class_of"]
            if lane_classes(data, base, bits).get(d, 0) != k:
                return False
    if "pairs" in case.claim and block_pairs(name, 3, data, base, 64) != case.claim["pairs"].get(finder(name, 3).min_dist):
        return False
    if "pairs_dyn" in case.claim and block_pairs(name, 8, data, base, 256) != case.claim["pairs_dyn"]:
        return False
    return True


_BUILT = {}


def build(name, what, make, salt):
    """make(seed) -> Case, redrawn until its claim holds in both variants.  (A case is a function of the row, its description and `salt`: built once for all qualities.)"""
    key = (name, what, salt)
    if key not in _BUILT:
        for k in range(400):
            case = make(zlib.crc32(("%s|%s|%d" % key).encode()) + k)
            if claim_holds(name, case, False) and (not case.end or claim_holds(name, case, True)):      # (a run BEHIND the buffer changes nothing in front of P)
                _BUILT[key] = case
                break
        else:
            raise AssertionError("no buffer for %s %s" % (name, what))
    return _BUILT[key]


# ------------------------------------------------------------------------------------------------ families
def k1(row, q):
    """One-distance classes of the wavefront [P, P + 64) (WAVEPOS).  The cursor reaches lane i over a copy that starts at P - a and is cut at P + i - 1."""
    name, f, out = row.name, finder(row.name, q), []
    ml = f.max_len
    a = 9 if ml >= 80 else 5                             # the copy in front of P: one token of a + i - 1 bytes (within max_len)

    def cut_case(what, i, m2, d=700, n_over=None, salt=0):
        """lane i proves: first mismatch of its candidate at P + m2 (None: none within 512 bytes); n_over: the stream ends n_over bytes behind lane i"""
        total = 600
        cuts = ([i - 1] if i else []) + ([m2] if m2 is not None else [])
        n_end = None if n_over is None else P0 + i + n_over

        def make(seed):
            data = copy_place(seed, d, a if i else 0, total, cuts, n_end=None if n_end is None else n_end + tail_skip(row))
            lanes = set(range(64 if n_end is None else min(64, n_end - 3 - P0))) - {c - k for c in cuts for k in range(4)}
            return Case("K1 " + what, data, P0 + i, end=n_end is not None, claim=dict(first=d, lane=i, class_of=(d, len(lanes))))
        out.append(build(name, what, make, salt))

    imax = min(12, ml - a + 1)
    # the first mismatch at every byte of a group of eight: lane i = 8 + off reads its own group from bit `off` on
    for i in range(8, imax):
        for m2 in range(i + 4, 16):
            cut_case("lane %d, first mismatch in its own group at byte %d" % (i, m2), i, m2, salt=i * 64 + m2)
    for m2 in range(16, 24):
        cut_case("lane 9, first mismatch in the next group at byte %d" % m2, 9, m2, salt=1000 + m2)
    for m2 in (40, 47, 48, 200, 455):
        cut_case("lane 9, first mismatch in a later group at byte %d" % m2, 9, m2, salt=1100 + m2)
    cut_case("lane 9, no mismatch within 512 bytes", 9, None, salt=1200)
    cut_case("lane 0, no mismatch within 512 bytes", 0, None, salt=1201)
    cut_case("lane 0, the distance is 3: the copy overlaps itself", 0, 300, d=3, salt=1202)
    # the stream ends inside [P, P + 512): n through all residues mod 8; a last, partial wavefront; n - pos = 447, 448, 449 for lanes of one wavefront
    for r in range(8):
        cut_case("lane 9, the stream ends %d bytes behind it" % (96 + r), 9, None, n_over=96 + r, salt=1300 + r)
    cut_case("lane 9 of a last wavefront of 30 positions", 9, None, n_over=24, salt=1320)
    for i, over in ((9, 449), (10, 448), (11, 447)):
        cut_case("lane %d, n - pos = %d" % (i, over), i, None, n_over=over, salt=1330 + i)

    # classes of exactly 7, 8 and 61 lanes: a copy of k + 3 bytes at P (k positions have four bytes of it); all 64 lanes: `lane 0, no mismatch within 512 bytes` above
    for k in (7, 8, 61):
        if k + 3 > ml:
            _no(row, q, "K1", "a class of %d lanes" % k, "one token holds at most %d bytes: the cursor would stand inside the class again" % ml)
            continue

        def make(seed, k=k):
            return Case("K1 a class of %d lanes" % k, copy_place(seed, 900, 0, k + 3, []), P0, claim=dict(first=900, lane=0, classes={900: k}))
        out.append(build(name, "class %d" % k, make, 1400 + k))

    # two classes of 8 and more lanes at different distances, and lanes without a candidate
    def make2(seed):
        bf = Buf(seed)
        bf.to(P0 - 1500); s1 = bf.text(12); bf.b += s1
        bf.to(P0 - 1100 + 20); s2 = bf.text(26); bf.b += s2
        bf.to(P0); bf.b[-1:] = FRONT; bf.b += s1[:11] + bytes([0x10]); bf.noise(7); bf.b += FRONT + s2[:23] + bytes([0x11]); bf.noise(200)
        return Case("K1 two classes: 8 lanes at 1500, 20 lanes at 1100", bytes(bf.b), P0 + 20, claim=dict(first=1100, lane=20, also=(P0, 1500), classes={1500: 8, 1100: 20}))
    if ml >= 23:
        out.append(build(name, "two classes", make2, 1500))
    else:
        def make2s(seed):
            bf = Buf(seed)
            bf.to(P0 - 1500); s1 = bf.text(12); bf.b += s1
            bf.to(P0 - 1100 + 20); s2 = bf.text(16); bf.b += s2
            bf.to(P0); bf.b[-1:] = FRONT; bf.b += s1[:11] + bytes([0x10]); bf.noise(7); bf.b += FRONT + s2[:13] + bytes([0x11]); bf.noise(200)
            return Case("K1 two classes: 8 lanes at 1500, 10 lanes at 1100", bytes(bf.b), P0 + 20, claim=dict(first=1100, lane=20, also=(P0, 1500), classes={1500: 8, 1100: 10}))
        out.append(build(name, "two classes", make2s, 1500))

    # a class whose distance exceeds the position of lane 0: the wavefront [64, 128), the copy at 84 from position 0
    def make3(seed):
        bf = Buf(seed)
        s = bf.text(84)
        bf.b += s + s[:47] + bytes([0x10])
        bf.to(P0 + 200)
        return Case("K1 44 lanes at distance 84 in the wavefront of position 64", bytes(bf.b), 84, start=True, claim=dict(first=84, lane=20, classes={84: 44}))
    out.append(build(name, "class in front of the stream", make3, 1600))
    return out


def k2(row, q):
    """PRUNE (from a best length of 16 on, the eight bytes that end at best_l) and ties (the first candidate of the best score wins)."""
    name, f, out = row.name, finder(row.name, q), []
    ml, mc = f.max_len, f.max_chain
    longer = min(40, ml)

    def add(what, lens, target_len=None, salt=0, **kw):
        if len(lens) > mc:
            _no(row, q, "K2", what, "maxChain is %d: the walk ends before the last of %d candidates" % (mc, len(lens)))
            return
        tl = target_len if target_len is not None else max(lens) + 6

        def make(seed):
            data, p, cands = place(seed, lens, tl, **kw)
            return Case("K2 " + what, data, p, cands, end=kw.get("tail") == 0)
        out.append(build(name, what, make, salt))

    for first in (15, 16, 17):
        if first >= longer:
            _no(row, q, "K2", "a first candidate of %d bytes, then a longer one" % first, "the longest match has %d bytes" % ml)
            continue
        add("a first candidate of %d bytes, then one of %d" % (first, longer), [first, longer], salt=first)
        # ... and between them one that agrees with the position up to best_l - 8 and differs inside the eight checked bytes
        for back in (1, 4, 7):
            add("%d bytes, then %d (differs %d in front of best_l), then %d" % (first, first - back, back, longer), [first, first - back, longer], salt=100 + first * 8 + back)
    # two candidates of equal length: the nearer wins; a third, shorter one in front
    for ln in sorted({8, min(17, ml), min(33, ml)}):
        add("two candidates of %d bytes" % ln, [ln, ln], salt=200 + ln)
        add("one of 5 bytes, then two of %d" % ln, [5, ln, ln], salt=240 + ln)
    # equal lengths as the last two steps of a full chain.  (Both are measured in the block's one final work_off(): the block lists a few dozen pairs.  Equal
    # candidates on both sides of a work_off() are K5's runs.)
    if mc >= 8:
        add("%d candidates of 6 bytes, then two of 20" % (mc - 2), [6] * (mc - 2) + [min(20, ml)] * 2, salt=300, gap=5)
    # a candidate of best_possible length ends the walk, a longer-looking one behind it
    if ml <= 300:
        add("the first candidate has max_len bytes, the second more", [ml + 20, ml + 30], target_len=ml + 40, salt=400, gap=12)
        add("one of 9 bytes, then max_len + 20, then max_len + 30", [9, ml + 20, ml + 30], target_len=ml + 40, salt=401, gap=12)
    else:
        _no(row, q, "K2", "a candidate of max_len bytes", "max_len is %s: the same through the stream's end" % ("unbounded" if ml >= G.INF else ml))
    add("the stream ends 60 bytes behind P: the first candidate has them all, the second too", [70, 80], target_len=60 + tail_skip(row), salt=410, tail=0)
    # CompatibilityMode cuts a length to the distance: periodic bytes at P (every row; the claim is MatchSearch restated)
    for period in (3, 5, 17):
        def make(seed, period=period):
            bf = Buf(seed)
            bf.to(P0)
            bf.b[-1:] = FRONT
            unit = bf.text(period)
            bf.b += (unit * 40)[:60] + bytes([0x10])
            bf.noise(200)
            return Case("K2 period %d for 60 bytes" % period, bytes(bf.b), P0 + period, claim=dict(first=period, lane=period))
        out.append(build(name, "period %d" % period, make, 500 + period))
    return out


def k3(row, q):
    """The compare cap of kernel B (48 or 256 in the regular pipeline): lengths cap - 1, cap, cap + 1 at the cursor and as the lazy neighbour; a match of
    exactly cap bytes that ends the stream; a capped candidate behind an uncapped better one."""
    name, f, out = row.name, finder(row.name, q), []
    caps = [c for c in (48, 256) if f.max_len > c]
    if b_cap(row, q) is None:
        _no(row, q, "K3", "the regular pipeline's cap", "max_len is %d: choose_b_cap gives no cap below 96" % f.max_len if f.max_len < 96 else "max_len does not exceed the cap")
    for cap in caps:                                     # (both numbers at every quality: the quality's own is b_cap(row, q), the other one is ALZ_SPEC_BCAP_SHORT's or a plain long match)
        for ln in (cap - 1, cap, cap + 1):
            for lazy in (False, True):
                what = "a candidate of %d bytes (cap %d)%s" % (ln, cap, ", P is the lazy neighbour" if lazy else "")
                if lazy and f.lazy < 4:
                    _no(row, q, "K3", what, "lazy is %d: a hash of four bytes finds no match of three for P - 1 (LzChainMatchFinder.cs:288-299)" % f.lazy)
                    continue

                def make(seed, ln=ln, lazy=lazy, what=what):
                    data, p, cands = place(seed, [ln], ln + 6, decoy=lazy)
                    return Case("K3 " + what, data, p, cands, claim=dict(lazy=lazy))
                out.append(build(name, what, make, cap * 8 + ln % 8 + (4 if lazy else 0)))

        def make_end(seed, cap=cap):
            data, p, cands = place(seed, [cap + 12], cap + tail_skip(row), tail=0)
            return Case("K3 a match of exactly %d bytes ends the stream" % cap, data, p, cands, end=True)
        out.append(build(name, "cap ends stream %d" % cap, make_end, cap * 8 + 3000))
        if f.max_chain >= 2:
            def make_behind(seed, cap=cap):
                data, p, cands = place(seed, [30, cap + 20], cap + 26)
                return Case("K3 one of 30 bytes, then one of %d (cap %d)" % (cap + 20, cap), data, p, cands)
            out.append(build(name, "capped behind %d" % cap, make_behind, cap * 8 + 3001))

            def make_front(seed, cap=cap):
                data, p, cands = place(seed, [cap + 20, cap + 30], cap + 40)
                return Case("K3 one of %d bytes, then one of %d (cap %d)" % (cap + 20, cap + 30, cap), data, p, cands)
            out.append(build(name, "capped in front %d" % cap, make_front, cap * 8 + 3002))
    return out


def k4(row, q):
    """The attempt count: M short candidates in front of the one long candidate, M = maxChain - 1 (found) and maxChain (not found); with a distance-1 candidate
    among them where min_distance is 2; the long candidate at max_dist and at max_dist + 1."""
    name, f, out = row.name, finder(row.name, q), []
    mc, long_len = f.max_chain, min(44, f.max_len)
    for m in (mc - 1, mc):
        def make(seed, m=m):
            data, p, cands = place(seed, [8] * m + [long_len], long_len + 6, gap=4)
            return Case("K4 %d candidates of 8 bytes in front of one of %d" % (m, long_len), data, p, cands, claim=dict(found=m < mc))
        out.append(build(name, "attempts %d" % m, make, 10 + m))
    if f.min_dist == 2:
        for m in (mc - 1, mc):
            what = "a distance-1 candidate and %d of 8 bytes in front of one of %d" % (m - 1, long_len)
            if f.lazy < 4:
                _no(row, q, "K4", what, "lazy is %d: position P - 1 has P's word and takes a match of four bytes, the cursor never stands on P" % f.lazy)
                continue

            def make(seed, m=m, what=what):
                W = bytes([1 + seed % 15]) * 4
                data, p, cands = place(seed, [8] * (m - 1) + [long_len], long_len + 6, gap=4, before=FRONT + W[:1], W=W)
                return Case("K4 " + what, data, p, [(p - 1, 4)] + cands, claim=dict(found=m < mc, lazy=True))
            out.append(build(name, what, make, 50 + m))
    if f.max_dist > 0x1000:
        _no(row, q, "K4", "the candidate at max_dist and max_dist + 1", "a window of %d bytes: left to the plants of tests/geometry_cases.py at max_dist - 1, max_dist and max_dist + 1 of every row, "
            "which run through the same four paths" % f.max_dist)
    if f.max_dist <= 0x1000:
        for over in (0, 1):
            def make(seed, over=over):
                data, p, cands = place(seed, [long_len], long_len + 6, dists={0: f.max_dist + over})
                return Case("K4 the candidate at max_dist%s" % (" + 1" if over else ""), data, p, cands, claim=dict(found=not over))
            out.append(build(name, "max_dist %d" % over, make, 90 + over))
    return out


def s_(row, q):
    """The scan search (benc_wave_scan_search, benc_scan_measure): 4 / 2 / 1 lanes per candidate at up to 16 / 32 / more candidates of one block of 1 024 positions
    behind the cursor; attempts that run out in the second block; the best candidate in the third block (LZ4 blocks: behind ALZ_SCAN_NEAR = 2 blocks, through the
    links).  The `lo` cut is K4's candidate at max_dist and max_dist + 1, the block that starts in front of the stream K1's wavefront of position 64."""
    name, f, out = row.name, finder(row.name, q), []
    if name not in SCAN_ROWS or not (q in SCAN_QUALITIES or (q == 10 and name in SCAN_Q10_ROWS)):
        return out
    mc, long_len = f.max_chain, min(44, f.max_len)
    for total in (16, 17, 24, 32):                       # candidates in ONE block, the best one last (32: the last count with two lanes per candidate, all 64 lanes busy)
        what = "%d candidates in one block, the last one has %d bytes" % (total, long_len)
        if total > mc:
            if total == 32 and name not in SCAN_Q10_ROWS:
                _no(row, q, "S", what, "maxChain 32 is quality 10, where this row's finder (min_len %d < 4) has the min-length table and takes_scan_path refuses it: quality 9, maxChain 24, is its most" % f.min_len)
            else:
                _no(row, q, "S", what, "maxChain is %d: the search lists no more candidates than that" % mc)
            continue

        def make(seed, total=total, what=what):
            data, p, cands = place(seed, [8] * (total - 1) + [long_len], long_len + 6, gap=4)
            assert p - cands[-1][0] < 1024
            return Case("S " + what, data, p, cands, claim=dict(found=True))
        out.append(build(name, what, make, 700 + total))
    _no(row, q, "S", "33 candidates in one block", "takes_scan_path wants maxChain <= 32 and benc_wave_scan_search clamps nc to 32: one lane per candidate (gsh 0) is never taken")
    for m in (mc - 1, mc):                               # half of the short candidates in the first block, the others and the long one in the second
        near = m // 2

        def make(seed, m=m, near=near):
            data, p, cands = place(seed, [8] * m + [long_len], long_len + 6, gap=4, dists={near: 1024 + 40})
            assert p - cands[near - 1][0] < 1024 < p - cands[near][0] and p - cands[-1][0] < 2048
            return Case("S %d candidates of 8 bytes in the first block, %d and the one of %d in the second" % (near, m - near, long_len), data, p, cands, claim=dict(found=m < mc))
        out.append(build(name, "edge %d" % m, make, 720 + m))
    if mc >= 3:
        def make(seed):
            data, p, cands = place(seed, [8, 8, long_len], long_len + 6, dists={1: 1500, 2: 2600})
            return Case("S the best candidate in the third block, one in the first and one in the second", data, p, cands, claim=dict(found=True))
        out.append(build(name, "third block", make, 740))
    return out


def k5(row, q):
    """The dense list (enc_match_dense_kernel: ALZ_DENSE_LIST = 256 pairs, work_off() in the middle of a walk): a run of one byte value through a whole block --
    every position of the run has maxChain candidates at distances 1, 2, 3, ... which all reach as far as the position can, so the nearest must win whichever
    side of a work_off() it was listed on (from maxChain 8 on the list of 256 pairs overflows every few trips of a block of 256 positions: these runs are the cases
    where equal candidates of one position are measured in different work_off() calls).  The run starts 8, 4, 3, 2 and 0 bytes in front of the block: at maxChain 4 the block of 64 positions lists 256, 256,
    255, 253 and 246 pairs.  Runs with background between them: positions without a candidate between positions with full chains (the lane refill of DYN).
    The stream ending 1, 63, 64 and 65 positions into a block."""
    name, out = row.name, []

    def run_case(what, start, pieces, n_end=None, salt=0, pairs=False):
        def make(seed):
            bf = Buf(seed)
            bf.to(P0 + start)
            bf.b[-1:] = FRONT
            for k, (run, gap) in enumerate(pieces):
                bf.b += bf.W[:1] * run
                if gap:
                    bf.b += bytes([0x10 + k % 10]); bf.noise(gap - 1)
            if n_end is None:
                bf.b += bytes([0x1B]); bf.noise(200)
            else:
                del bf.b[n_end + tail_skip(row):]
            claim = dict(first=1, lane=start + 1)
            if pairs:                                    # the 64 positions of the block [P, P + 64) at maxChain 4: distances 1 .. min(4, x - s), those from min_dist on listed
                claim["pairs"] = {md: sum(max(0, min(4, x - start) - (md - 1)) for x in range(64)) for md in (1, 2)}
            return Case("K5 " + what, bytes(bf.b), P0 + start + 1, end=n_end is not None, claim=claim)
        out.append(build(name, what, make, salt))

    for start in (-8, -4, -3, -2, 0):
        run_case("a run of 600 bytes from %d bytes in front of the block" % -start, start, [(600, 0)], salt=600 - start, pairs=True)
    if finder(name, 3).min_dist > 1:
        _no(row, q, "K5", "255 and 256 pairs in a block of 64 positions", "min_distance is %d: distance 1 spends its attempt and is not listed, the block lists at most 192 pairs (183 .. 192 are built)" % finder(name, 3).min_dist)
    # exactly 257 pairs in a block of 256 positions at maxChain 16: sixteen positions of one class inside the block, each with sixteen and more earlier positions of the
    # class -- sixteen of them in front of the block -- list 256; one position of a second class with one earlier occurrence lists the pair that does not fit
    # (`ln + k > ALZ_DENSE_LIST`).  Every occurrence is the word and a byte of its own, so no other word repeats; the background is redrawn until no position of the
    # block collides.  All sixteen candidates of P have four bytes: the nearest wins.
    if finder(name, q).max_chain == 16:
        def make257(seed):
            bf = Buf(seed)
            V = bytes(bf.W[::-1])
            bf.to(P0 - 300); bf.b += V + b"\x10"
            for k in range(32):
                bf.to(P0 - 128 + 8 * k)
                if k == 16:                                # (P: the byte in front must not lengthen a match)
                    bf.b[-1:] = FRONT
                bf.b += bf.W + bytes([0x40 + k])
            bf.to(P0 + 200); bf.b += V + b"\x11"
            bf.to(P0 + 456)
            return Case("K5 exactly 257 pairs in the block of 256 positions", bytes(bf.b), P0, [(P0 - 8 * (k + 1), 4) for k in range(16)], claim=dict(pairs_dyn=257))
        out.append(build(name, "257 pairs", make257, 690))
    else:
        _no(row, q, "K5", "exactly 257 pairs", "a block of 64 positions with 4 candidates each (maxChain 4) lists at most 256; the case is built for the blocks of 256 positions at maxChain 16 (quality 8): "
            "sixteen positions with full chains and one pair more")
    run_case("five runs of 40 bytes with 24 background bytes between them", 0, [(40, 24)] * 5, salt=620)
    for k in (1, 63, 64, 65):
        for block in (64, 256):                          # the stream's last block holds k positions: limit = P + 256 + block' + k - 1
            base = P0 + 256 + (block if block == 64 else 0)
            run_case("a run to the stream's end, %d positions in the last block of %d" % (k, block), -8, [(base - P0 + 8 + k + 3, 0)], n_end=base + k + 3, salt=640 + k + block)
    return out


def n_(row, q):
    """Narrowing (enc_narrow_lds_kernel, enc_narrow_kernel): j = 0 .. 5 positions between P and its true predecessor whose words collide with P's at 15 bits and
    not at the finder's width; the predecessor at max_dist and max_dist + 1 behind two collisions; P at 0 and 1 past the range edges 4096 and 8192 with
    its predecessor in front of the edge.  The chain at the finder's width is the one candidate whatever the collisions: the claim is K4's."""
    name, f, out = row.name, finder(row.name, q), []
    if f.hash_bits <= 15 or f.props is not None or f.max_dist > 0xFFFF:
        _no(row, q, "N", "all", "narrows_links: 16-bit links, one property set, a hash wider than 15 bits")
        return out
    long_len = min(44, f.max_len)
    if f.max_dist > 8192:
        _no(row, q, "N", "these cases through enc_narrow_kernel", "in a 64 KiB window enc_words_kernel sends only streams of FEW distinct words to the narrowing; these backgrounds are random bytes and go "
            "through kernel A's passes.  The `collide` batch of words_batches() carries a built collision through enc_narrow_kernel")
    for j in range(6):
        def make(seed, j=j):
            data, p, cands = place(seed, [long_len], long_len + 6, collide=j)
            return Case("N %d collisions at 15 bits in front of the predecessor" % j, data, p, cands, claim=dict(found=True, collide=j))
        out.append(build(name, "collide %d" % j, make, 800 + j))
    if f.max_dist <= 0x1000:
        for over in (0, 1):
            def make(seed, over=over):
                data, p, cands = place(seed, [long_len], long_len + 6, dists={0: f.max_dist + over}, collide=2)
                return Case("N the predecessor at max_dist%s behind 2 collisions" % (" + 1" if over else ""), data, p, cands, claim=dict(found=not over, collide=2))
            out.append(build(name, "collide max_dist %d" % over, make, 810 + over))
    for P in (4096, 4097, 8192, 8193):
        def make(seed, P=P):
            data, p, cands = place(seed, [long_len], long_len + 6, collide=2, P=P, tail=P0 - P + 200)
            return Case("N P = %d, 2 collisions" % P, data, p, cands, claim=dict(found=True, collide=2, lane=P % 256))
        out.append(build(name, "edge %d" % P, make, 820 + P % 7))
    return out


BUILDERS = dict(K1=k1, K2=k2, K3=k3, K4=k4, K5=k5, N=n_, S=s_)


@functools.lru_cache(maxsize=None)
def cases(name, q, family):
    """the cases of (row, quality, family) -- built once, shared, never changed"""
    return tuple(BUILDERS[family](G.BY_NAME[name], q))


def families_of(name, q):
    return FAMILIES if q in QUALITIES and name not in S_ONLY else ("S",)


def all_cases(name, q):
    return [c for fam in families_of(name, q) for c in cases(name, q, fam)]


# (qualities 9 and 10, and every quality of raw Snappy: family S alone)
PAIRS = [(name, q) for name in ROWS if name not in S_ONLY for q in QUALITIES] + [(name, 9) for name in SCAN_ROWS if name not in S_ONLY] + [(name, q) for name in S_ONLY for q in SCAN_QUALITIES] + [(name, 10) for name in SCAN_Q10_ROWS]


def build_all():
    for name, q in PAIRS:
        all_cases(name, q)
    return NOT_EXPRESSIBLE


# ------------------------------------------------------------------------------------------------ K6: the probe's own streams
def _small(rng, run_len, noise_len):
    return (RUN * (run_len // 2 + 1))[:run_len] + rng.integers(0x20, 0x100, noise_len, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def probe_batch():
    """600 streams for the lane side (the list of enc_match_kernel goes round its 512 rows) mixed with 50 for the dense side, about 300 bytes each; and streams
    whose `limit` is 63 (the probe answers 0 without looking) and 64.  -> [(raw, side or None)]"""
    rng = np.random.default_rng(66)
    out = []
    for i in range(650):
        dense = i % 13 == 5
        n = 280 + int(rng.integers(0, 40))
        out.append((_small(rng, 16, n - 16), False) if dense else (_small(rng, n - 80 - n % 2, 80 + n % 2), True))
    for limit in (63, 64):
        out.append((_small(rng, limit + 4 - 10, 10), None if limit < 64 else True))
        out.append((_small(rng, 0, limit + 4), None if limit < 64 else False))
    return out


@functools.lru_cache(maxsize=None)
def probe_line():
    """Streams exactly on the probe's line and one hit below it: 1 100 bytes, so step is 1 and the samples are positions 0 .. 1023 (tot = 1024); a run of L bytes
    of period 2 at the start hits at positions 2 .. L - 16: L = 273 gives 256 = tot / 4 hits (the lane side), L = 272 gives 255.  -> [(raw, hits)]"""
    rng = np.random.default_rng(67)
    return [((RUN * 200)[:L] + rng.integers(0x20, 0x100, 1100 - L, dtype=np.uint8).tobytes(), L - 17) for L in (273, 272, 274, 271)]


# ------------------------------------------------------------------------------------------------ K7: the words choice
def words_counts(name, q, data):
    """enc_words_kernel restated -> (distinct, tot, narrow): the distinct `>> 17` hashes of four windows of 1 024 positions at 1 / 8, 3 / 8, 5 / 8 and 7 / 8 of the
    stream, each window counted by itself; few = distinct * 16 < tot * thresh, 4 for 64 KiB windows (narrow the FEW), 11 and inverted for windows up to 8 KiB with
    the min-length table (narrow the MANY); nothing narrows below 256 sampled positions."""
    row, f = G.BY_NAME[name], finder(name, q)
    limit = len(data) - tail_skip(row) - 4
    h = (hashes(data[:limit + 4], 15)).tolist() if limit >= 0 else []
    fresh = tot = 0
    for k in range(4):
        base = (limit + 1) * (2 * k + 1) // 8
        win = h[base:min(base + 1024, limit + 1)]
        fresh += len(set(win)); tot += len(win)
    winm = f.max_dist <= 8192 and f.min_table is not None
    few = fresh * 16 < tot * (11 if winm else 4)
    return fresh, tot, tot >= 256 and (not few if winm else few)


@functools.lru_cache(maxsize=None)
def words_batches():
    """-> {name: [raw]}: `split` 2 048 + 64 streams of 1.5 .. 3 KiB, every other one of two byte values (few distinct words) and of 224 (many): from
    ALZ_NARROW_SPLIT_MIN = 2 048 streams on the choice is per stream; `few` and `many`: 100 such streams with a majority of 60 either way (enc_words_merge_kernel
    sends all the majority's way); `collide`: the same with the 60 built of two words that collide at 15 bits; `short`: streams with fewer than 256 sampled positions, and just enough."""
    rng = np.random.default_rng(77)

    def stream(few, n=None):
        n = n or int(rng.integers(1536, 3072))
        return rng.integers(0x30, 0x32 if few else 0x100, n, dtype=np.uint8).tobytes()
    W = bytes([1, 2, 3, 4])
    C = colliders(W, 1, 78)[0]

    def two_words():
        """few distinct words, two of which collide at 15 bits and not at 16: the narrowing walk of a 64 KiB window meets the collision"""
        return b"".join(W if x else C for x in rng.integers(0, 2, int(rng.integers(384, 768))))
    return dict(split=[stream(i % 2 == 0) for i in range(2048 + 64)], few=[stream(i % 5 < 3) for i in range(100)], many=[stream(i % 5 >= 3) for i in range(100)],
                collide=[two_words() if i % 5 < 3 else stream(False) for i in range(100)],
                short=[stream(i % 2 == 0, n) for n in (100, 128, 129, 130, 131, 140) for i in range(2)])


def few_words(raw):
    """how a stream of words_batches was drawn: of two byte values, or of the two colliding words"""
    return len(set(raw)) <= 8


WORDS_PAIRS = (("lz4_block", 8), ("yaz0", 12))      # 64 KiB windows; windows up to 8 KiB with the min-length table (the inverted threshold)
