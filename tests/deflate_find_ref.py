"""Pure-Python restatement of the DEFLATE encoder (alz_deflate_*): alz_deflate_find_kernel and alz_deflate_emit_kernel of csrc/alz_inflate.hip
and the code builder of csrc/alz_inflate.h.  TEST-ONLY.  The BCL's bytes are no contract for this encoder, so its yardstick is its own
specification -- "the chains, and with them the tokens, are a function of the stream's bytes and the level alone" -- restated here step by
step and held bit for bit against the GPU (tests/test_gpu_deflate_find.py).  It follows the kernel, not an ideal finder, and reproduces:

* Two DIFFERENT trigrams of one step in one hash bucket both link to the old head, and the later one becomes the head: the earlier one
  is on no later chain unless a later lane of that step carries its trigram (the collision bypass).
* All 64 lanes write their slot of `prev` before any lane walks, so the slot of a candidate 32 768 - 63 .. 32 768 back may already hold
  the link of a position of the current step.
* Every lane with three bytes left in the STREAM is inserted, whatever the block's end (a block that is not the last is 511 whole steps,
  and in the last block bend == n, so no inserted position lies behind `bend`; bend - 2 and bend - 1 of a block that is not the last are
  inserted although they can start no match).
* The lazy rule looks at the next lane of the same step only: lane 63 is never turned into a literal.

One liberty, for speed: a lane's walk reads only what is fixed for the whole step (src, and `prev` as the 64 writes left it), so the walk of
a position runs when the parse asks for it (`every=True` runs all 64, as the kernel does).

find(src, k, level) -> the tokens of block k: ("lit", byte) / ("match", length, distance).
plan(lit_freq, dist_freq, raw_len, ntok, final, stored_only, fixed_only) -> alz_deflate_plan_block's result as a dict.
emit(src, bs, blen, final, tokens, p) -> the block's bytes.  encode(src, level, flags) -> the stream.  blocks(src, level, flags) -> per block
its start, its tokens, its plan and its bytes."""

BLOCK = 32704                 # ALZ_DEFLATE_BLOCK
WIN = 32768                   # DFL_WIN
HASH_BITS = 14                # DFL_HASH_BITS
NLIT, NDIST, NCL = 286, 30, 19
STORED, FIXEDB, DYNAMIC = 0, 1, 2
FIXED_FLAG = 1                # ALZ_DEFLATE_FIXED
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------- alz_deflate_level_*
def level_chain(level):
    return 4 if level <= 1 else 8 if level == 2 else 16 if level <= 4 else 32 if level == 5 else 64 if level == 6 else 128 if level == 7 else 256 if level == 8 else 1024


def level_nice(level):
    return 32 if level <= 1 else 64 if level == 2 else 128 if level <= 4 else 258


def level_lazy(level):
    return level >= 4


# ---------------------------------------------------------------------------------------------- the symbol tables, as the header's arithmetic
def len_sym(length):
    """-> (symbol, extra bits, their value)"""
    l = length - 3
    if l < 8:
        return 257 + l, 0, 0
    if length == 258:
        return 285, 0, 0
    e = l.bit_length() - 1 - 2
    return 261 + 4 * e + ((l >> e) & 3), e, l & ((1 << e) - 1)


def len_extra(sym):
    return 0 if sym < 265 or sym == 285 else (sym - 261) >> 2


def dist_sym(dist):
    d = dist - 1
    if d < 4:
        return d, 0, 0
    k = d.bit_length() - 1
    e = k - 1
    return 2 * k + ((d >> e) & 1), e, d & ((1 << e) - 1)


def dist_extra(sym):
    return 0 if sym < 4 else (sym >> 1) - 1


def fixed_len(sym):
    return 8 if sym < 144 else 9 if sym < 256 else 7 if sym < 280 else 8


def trigram_hash(tri):
    return ((tri * 0x9E3779B1) & M32) >> (32 - HASH_BITS)


# ---------------------------------------------------------------------------------------------- find
def match_len(src, a, b, maxlen):
    """dfl_match_len: equal bytes at a and b, at most maxlen"""
    if src[a:a + maxlen] == src[b:b + maxlen]:
        return maxlen
    i = 0
    while src[a + i] == src[b + i]:
        i += 1
    return i


def find_all(src, k, level, every=False):
    """-> (tokens, best): the tokens of block k and, per position of the block whose walk ran, its (length, distance) with length 0 for
    "no match".  The body of `if (level > 0 && blen > 0)` of alz_deflate_find_kernel."""
    n = len(src)
    bs = k * BLOCK
    blen = min(n - bs, BLOCK)
    bend = bs + blen
    tokens, best_of = [], {}
    if level <= 0 or blen <= 0:
        return tokens, best_of
    head = [0] * (1 << HASH_BITS)                  # the newest position + 1 per hash
    prev = [0] * WIN                               # per position mod 32 Ki: the distance to the one before it on its chain; 0 ends it
    chain_max, nice, lazy = level_chain(level), level_nice(level), level_lazy(level)
    skip = 0
    gs = bs - WIN if bs > WIN else 0
    while gs < bend:
        # ---- the step's 64 positions: hash, read the heads, link, write prev for ALL lanes, then publish the heads
        hashable, hs, delta = [False] * 64, [0] * 64, [0] * 64
        nearest = {}                               # trigram -> the last lane so far that has it
        for lane in range(64):
            p = gs + lane
            if p + 3 > n:
                continue
            hashable[lane] = True
            tri = src[p] | (src[p + 1] << 8) | (src[p + 2] << 16)
            h = hs[lane] = trigram_hash(tri)
            old = head[h]                          # (no lane of this step has published yet)
            d = 0
            if tri in nearest:                     # the nearest EARLIER LANE with the same three bytes ...
                d = lane - nearest[tri]
            elif old:                              # ... else the old head
                d = p + 1 - old
            if d > WIN:
                d = 0
            delta[lane] = d
            nearest[tri] = lane
        for lane in range(64):
            if hashable[lane]:
                prev[(gs + lane) & (WIN - 1)] = delta[lane]
        for lane in range(64):
            if hashable[lane] and gs + lane + 1 > head[hs[lane]]:
                head[hs[lane]] = gs + lane + 1     # atomicMax
        if gs < bs:                                # the window in front of the block: inserted only
            gs += 64
            continue

        # ---- the best match of a position
        memo = {}

        def walk(lane):
            if lane in memo:
                return memo[lane]
            p = gs + lane
            maxlen = min(bend - p, 258) if p < bend else 0
            best = best_dist = 0
            if maxlen >= 3 and hashable[lane]:
                cur, dl, c = p, delta[lane], chain_max
                while dl and c:
                    if dl > cur:
                        break
                    cur -= dl
                    dist = p - cur
                    if dist > WIN:
                        break
                    if best < 3 or src[cur + best] == src[p + best]:
                        ln = match_len(src, cur, p, maxlen)
                        if ln > best:
                            best, best_dist = ln, dist
                        if best >= nice or best >= maxlen:
                            break
                    dl = prev[cur & (WIN - 1)]
                    c -= 1
                if best < 3 or (best == 3 and best_dist > 4096):
                    best = 0
            memo[lane] = (best, best_dist)
            if p < bend:
                best_of[p] = memo[lane]
            return memo[lane]

        nvalid = min(bend - gs, 64)
        if every:
            for lane in range(64):
                walk(lane)
        # ---- the parse of these 64 positions
        cur = skip
        while cur < nvalid:
            L, D = walk(cur)
            if lazy and L >= 3 and cur + 1 < nvalid and walk(cur + 1)[0] > L:
                L = 0
            if L < 3:
                tokens.append(("lit", src[gs + cur]))
                cur += 1
            else:
                tokens.append(("match", L, D))
                cur += L
        skip = cur - nvalid
        gs += 64
    return tokens, best_of


def find(src, k, level):
    return find_all(src, k, level)[0]


def histograms(tokens):
    """the two LDS histograms as lane 0 sees them: the end-of-block's 1 is in"""
    lit_freq, dist_freq = [0] * NLIT, [0] * NDIST
    for t in tokens:
        if t[0] == "lit":
            lit_freq[t[1]] += 1
        else:
            lit_freq[len_sym(t[1])[0]] += 1
            dist_freq[dist_sym(t[2])[0]] += 1
    lit_freq[256] = 1
    return lit_freq, dist_freq


# ---------------------------------------------------------------------------------------------- the code builder
def build_lengths(freq, n, limit):
    """alz_deflate_build_lengths"""
    lens = [0] * n
    order = []                                     # the used symbols by (count, symbol): an insertion sort that never passes an equal count
    for i in range(n):
        if not freq[i]:
            continue
        j = len(order)
        order.append(i)
        while j > 0 and freq[order[j - 1]] > freq[i]:
            order[j] = order[j - 1]
            j -= 1
        order[j] = i
    m = len(order)
    if m == 0:
        return lens
    if m == 1:
        lens[order[0]] = 1
        return lens
    w = [freq[s] for s in order] + [0] * (m - 1)
    par = [0] * (2 * m - 1)
    a, b = 0, m                                    # the next leaf, the next inner node
    for t in range(m, 2 * m - 1):
        total = 0
        for _ in range(2):
            if a < m and (b >= t or w[a] <= w[b]):
                x = a
                a += 1
            else:
                x = b
                b += 1
            total += w[x]
            par[x] = t
        w[t] = total
    root = 2 * m - 2
    par[root] = 0                                  # par[] turns into depths
    for i in range(root - 1, -1, -1):
        par[i] = par[par[i]] + 1
    blc = [0] * 16
    for j in range(m):
        blc[min(par[j], limit)] += 1
    kraft = sum(blc[d] << (limit - d) for d in range(1, limit + 1))
    while kraft > (1 << limit):
        d = limit - 1
        while not blc[d]:
            d -= 1
        blc[d] -= 1
        blc[d + 1] += 2
        blc[limit] -= 1
        kraft -= 1
    j = 0
    for d in range(limit, 0, -1):
        for _ in range(blc[d]):
            lens[order[j]] = d
            j += 1
    return lens


def codes(lens):
    """alz_deflate_codes: canonical codes, BIT-REVERSED"""
    blc = [0] * 16
    for l in lens:
        blc[l] += 1
    code, blc[0] = 0, 0
    for d in range(1, 16):
        cnt = blc[d]
        code <<= 1
        blc[d] = code
        code += cnt
    out = []
    for l in lens:
        if not l:
            out.append(0)
            continue
        c, r = blc[l], 0
        blc[l] += 1
        for _ in range(l):
            r = (r << 1) | (c & 1)
            c >>= 1
        out.append(r)
    return out


class Bits:
    """LSB first"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, k):
        self.v |= (v & ((1 << k) - 1)) << self.n
        self.n += k

    def tobytes(self):
        return self.v.to_bytes((self.n + 7) >> 3, "little")


def run_lengths(lit_len, dist_len):
    """alz_deflate_run_lengths -> (hlit, hdist, [(symbol 0..18, value of its extra bits)])"""
    hlit, hdist = NLIT, NDIST
    while hlit > 257 and not lit_len[hlit - 1]:
        hlit -= 1
    while hdist > 1 and not dist_len[hdist - 1]:
        hdist -= 1
    allv = list(lit_len[:hlit]) + list(dist_len[:hdist])
    total, rl, i = hlit + hdist, [], 0
    while i < total:
        v, run = allv[i], 1
        while i + run < total and allv[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                c = min(run, 138)
                rl.append((18, c - 11))
                run -= c
            if run >= 3:
                rl.append((17, run - 3))
                run = 0
        else:
            rl.append((v, 0))
            run -= 1
            while run >= 3:
                c = min(run, 6)
                rl.append((16, c - 3))
                run -= c
        rl += [(v, 0)] * run
    return hlit, hdist, rl


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def header(lit_len, dist_len):
    """alz_deflate_header -> (bits, bytes)"""
    hlit, hdist, rl = run_lengths(lit_len, dist_len)
    cl_freq = [0] * NCL
    for s, _ in rl:
        cl_freq[s] += 1
    cl_len = build_lengths(cl_freq, NCL, 7)
    cl_code = codes(cl_len)
    hclen = NCL
    while hclen > 4 and not cl_len[CL_ORDER[hclen - 1]]:
        hclen -= 1
    w = Bits()
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_len[CL_ORDER[i]], 3)
    for s, extra in rl:
        w.put(cl_code[s], cl_len[s])
        if s >= 16:
            w.put(extra, 2 if s == 16 else 3 if s == 17 else 7)
    return w.n, w.tobytes()


def block_bytes_of(bits, final):
    return (bits + 7) >> 3 if final else ((bits + 3 + 7) >> 3) + 4


def plan(lit_freq, dist_freq, raw_len, ntok, final, stored_only, fixed_only):
    """alz_deflate_plan_block (lit_freq holds the end-of-block's 1)"""
    p = dict(type=STORED, ntok=ntok, bits=8 * (5 + raw_len), hdr_bits=0, bytes=5 + raw_len, lit_len=[0] * 288, dist_len=[0] * 32, hdr=b"",
             size=[8 * (5 + raw_len), M32, M32])
    if stored_only:
        return p
    p["lit_len"] = build_lengths(lit_freq, NLIT, 15) + [0, 0]
    p["dist_len"] = build_lengths(dist_freq, NDIST, 15) + [0, 0]
    p["hdr_bits"], p["hdr"] = header(p["lit_len"], p["dist_len"])
    fixed, dyn = 3, 3 + p["hdr_bits"]
    for s in range(NLIT):
        e = len_extra(s) if s > 256 else 0
        fixed += lit_freq[s] * (fixed_len(s) + e)
        dyn += lit_freq[s] * (p["lit_len"][s] + e)
    for s in range(NDIST):
        e = dist_extra(s)
        fixed += dist_freq[s] * (5 + e)
        dyn += dist_freq[s] * (p["dist_len"][s] + e)
    p["size"][1], p["size"][2] = fixed, dyn
    if block_bytes_of(fixed, final) < p["bytes"]:
        p.update(type=FIXEDB, bits=fixed, bytes=block_bytes_of(fixed, final))
    if not fixed_only and block_bytes_of(dyn, final) < p["bytes"]:
        p.update(type=DYNAMIC, bits=dyn, bytes=block_bytes_of(dyn, final))
    return p


# ---------------------------------------------------------------------------------------------- emit
def emit(src, bs, blen, final, tokens, p):
    """alz_deflate_emit_kernel: the bytes of one block"""
    if p["type"] == STORED:
        return bytes([1 if final else 0, blen & 0xFF, blen >> 8, ~blen & 0xFF, (~blen >> 8) & 0xFF]) + bytes(src[bs:bs + blen])
    if p["type"] == DYNAMIC:
        lit_len, dist_len = p["lit_len"], p["dist_len"]
    else:
        lit_len, dist_len = [fixed_len(s) for s in range(288)], [5] * 32
    lit_code, dist_code = codes(lit_len), codes(dist_len)
    w = Bits()
    w.put((1 if final else 0) | (p["type"] << 1), 3)
    if p["type"] == DYNAMIC:
        w.put(int.from_bytes(p["hdr"], "little"), p["hdr_bits"])
    for t in tokens:
        if t[0] == "lit":
            w.put(lit_code[t[1]], lit_len[t[1]])
        else:
            ls, eb, ev = len_sym(t[1])
            w.put(lit_code[ls], lit_len[ls])
            w.put(ev, eb)
            ds, eb, ev = dist_sym(t[2])
            w.put(dist_code[ds], dist_len[ds])
            w.put(ev, eb)
    w.put(lit_code[256], lit_len[256])
    assert w.n == p["bits"], "the plan counted %d bits, the writer made %d" % (p["bits"], w.n)
    if final:
        out = w.tobytes()
    else:                                          # the joining: an empty stored block
        w.put(0, 3)
        out = w.tobytes() + b"\x00\x00\xff\xff"
    assert len(out) == p["bytes"]
    return out


def blocks(src, level, flags=0, tokens_of=None):
    """per block of the stream: dict(k, start, tokens, plan, bytes).  tokens_of(k): the block's tokens if the caller has them already."""
    src = bytes(src)
    n = len(src)
    out = []
    for k in range((n + BLOCK - 1) // BLOCK if n else 1):
        bs = k * BLOCK
        blen = min(n - bs, BLOCK)
        final = bs + blen == n
        tokens = tokens_of(k) if tokens_of else find(src, k, level)
        lit_freq, dist_freq = histograms(tokens)
        p = plan(lit_freq, dist_freq, blen, len(tokens), final, level == 0, bool(flags & FIXED_FLAG))
        out.append(dict(k=k, start=bs, tokens=tokens, plan=p, bytes=emit(src, bs, blen, final, tokens, p)))
    return out


def encode(src, level, flags=0):
    return b"".join(b["bytes"] for b in blocks(src, level, flags))


def bound(n):
    """alz_deflate_bound"""
    return n + 5 * ((n + BLOCK - 1) // BLOCK if n else 1)
