"""Pure Python, no zlib import: a bit-level ASSEMBLER of raw DEFLATE streams (RFC 1951) -- stored, fixed and dynamic blocks from token lists and
explicit code lengths, the malformed forms included -- and a REFERENCE DECODER that returns (status, output, src_used) by the frozen rules of
include/auroralz.h (zlib's inflate with window bits -15).  The decoder reads one bit at a time and resolves codes by canonical compare, so it
shares no table or buffer logic with the kernels.  tests/test_inflate_cpu.py holds it against the standard library."""

OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
NO_BOUND = 0xFFFFFF00

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_FLAT = [4] * 13 + [5] * 6                  # a complete code-length code that has all 19 symbols


# ---------------------------------------------------------------------------------------------- the assembler
class BitWriter:
    """bits go out LSB first; Huffman codes MSB first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)

    def align(self, fill=0):
        if self.n:
            self.put(fill, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += bytes(data)

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def bytes(self, fill=0):
        """the stream so far; the rest of the last byte is padding of either value"""
        if not self.n:
            return bytes(self.out)
        return bytes(self.out) + bytes([(self.acc | ((0xFF if fill else 0) << self.n)) & 0xFF])


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (0 = no code); the set need not be complete or even valid"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lens):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 is a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def flat_lens(symbols, n):
    """n code lengths: a complete code (two neighbouring lengths) over `symbols`; one symbol gets a single 1-bit code"""
    symbols = sorted(set(symbols))
    lens = [0] * n
    k = len(symbols)
    if k == 1:
        lens[symbols[0]] = 1
        return lens
    b = (k - 1).bit_length()
    short = (1 << b) - k
    for i, s in enumerate(symbols):
        lens[s] = b - 1 if i < short else b
    return lens


def length_symbol(length):
    """(symbol, extra bits, extra value) -- the usual choice (258 as symbol 285)"""
    assert 3 <= length <= 258
    i = max(j for j in range(29) if LEN_BASE[j] <= length)
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    assert 1 <= dist <= 32768
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def put_tokens(w, tokens, lit_codes, dist_codes, end=True):
    """tokens: ("lit", byte) | ("match", length, distance) | ("sym", literal/length symbol)  -- a bare symbol, nothing behind it --
    | ("len", symbol, extra value) | ("dist", symbol, extra value) -- the halves of a match spelled out -- | ("bits", value, n)"""
    for t in tokens:
        if t[0] == "lit":
            w.code(*lit_codes[t[1]])
        elif t[0] == "match":
            s, eb, ev = length_symbol(t[1])
            w.code(*lit_codes[s]); w.put(ev, eb)
            d, db, dv = dist_symbol(t[2])
            w.code(*dist_codes[d]); w.put(dv, db)
        elif t[0] == "sym":
            w.code(*lit_codes[t[1]])
        elif t[0] == "len":
            w.code(*lit_codes[t[1]]); w.put(t[2], LEN_EXTRA[t[1] - 257] if t[1] <= 285 else 0)
        elif t[0] == "dist":
            w.code(*dist_codes[t[1]]); w.put(t[2], DIST_EXTRA[t[1]] if t[1] < 30 else 0)
        elif t[0] == "bits":
            w.put(t[1], t[2])
        else:
            raise ValueError(t)
    if end:
        w.code(*lit_codes[256])


def stored_block(w, data, final, nlen=None, fill=0):
    w.put(1 if final else 0, 1); w.put(0, 2)
    w.align(fill)
    n = len(data)
    w.put(n, 16); w.put((n ^ 0xFFFF) if nlen is None else nlen, 16)
    w.raw(data)


def fixed_block(w, tokens, final, end=True):
    w.put(1 if final else 0, 1); w.put(1, 2)
    put_tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST), end)


def rle_lengths(lens):
    """the code-length symbols (symbol, extra value) that zlib-like run-length coding gives: 16 / 17 / 18 with maximal runs"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11)); run -= k
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out += [(0, 0)] * run
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3)); run -= k
            out += [(v, 0)] * run
        i = j
    return out


def dynamic_header(w, lit_lens, dist_lens, cl_syms=None, cl_lens=None, hclen=None, hlit=None, hdist=None):
    """HLIT / HDIST / HCLEN, the code-length code, the lengths.  lit_lens has 257..288 entries and dist_lens 1..32 (more than 286 / 30 only to
    write the malformed counts).  cl_syms: the code-length symbols as (symbol, extra value), default one symbol per length (no repeats);
    cl_lens: the 19 lengths of the code-length code, default CL_FLAT; hclen: how many of them are written (default: up to the last nonzero)."""
    cl_lens = list(CL_FLAT if cl_lens is None else cl_lens)
    if cl_syms is None:
        cl_syms = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    if hclen is None:
        hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
    w.put((len(lit_lens) - 257) if hlit is None else hlit, 5)
    w.put((len(dist_lens) - 1) if hdist is None else hdist, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl_codes = canonical(cl_lens)
    for s, ev in cl_syms:
        w.code(*cl_codes[s])
        if s >= 16:
            w.put(ev, (2, 3, 7)[s - 16])


def dynamic_block(w, tokens, final, lit_lens, dist_lens, end=True, **header):
    w.put(1 if final else 0, 1); w.put(2, 2)
    dynamic_header(w, lit_lens, dist_lens, **header)
    put_tokens(w, tokens, canonical(lit_lens), canonical(dist_lens), end)


def lens_for(tokens, with_end=True):
    """(lit_lens, dist_lens): complete flat codes over exactly the symbols the tokens use"""
    ls, ds = {256} if with_end else set(), set()
    for t in tokens:
        if t[0] == "lit":
            ls.add(t[1])
        elif t[0] == "match":
            ls.add(length_symbol(t[1])[0]); ds.add(dist_symbol(t[2])[0])
        elif t[0] in ("sym", "len"):
            ls.add(t[1])
        elif t[0] == "dist":
            ds.add(t[1])
    lit = flat_lens(ls, max(257, max(ls) + 1))
    dist = flat_lens(ds, max(ds) + 1) if ds else [0]
    return lit, dist


def expected(tokens):
    """what ("lit" / "match") tokens produce"""
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out)


# ---------------------------------------------------------------------------------------------- the reference decoder
class _Trunc(Exception):
    pass


class _Bad(Exception):
    pass


class _Full(Exception):
    pass


class _Bits:
    def __init__(self, src):
        self.src, self.pos = src, 0                   # pos in bits

    def left(self):
        return 8 * len(self.src) - self.pos

    def get(self, n):
        if self.left() < n:
            raise _Trunc
        v = 0
        for i in range(n):
            v |= ((self.src[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v


def _check_set(lens, codes_kind):
    """inflate_table's verdict: over-subscribed, or incomplete unless (not the code-length code and) the longest code is 1 bit"""
    used = [l for l in lens if l]
    if not used:
        return                                        # no code at all: accepted; every lookup finds an invalid 1-bit entry
    k = kraft(lens)
    if k > 32768:
        raise _Bad
    if k < 32768 and (codes_kind or max(used) != 1):
        raise _Bad


class _Code:
    def __init__(self, lens):
        self.by = {}
        for s, (c, l) in canonical(lens).items():
            self.by[(l, c)] = s
        self.maxl = max([l for l in lens if l], default=0)

    def read(self, bits):
        """one symbol; a code the set does not have is BAD_TOKEN once its bits are there (an empty set: after 1 bit)"""
        mark = bits.pos
        c = 0
        for l in range(1, max(self.maxl, 1) + 1):
            try:
                c = (c << 1) | bits.get(1)
            except _Trunc:
                bits.pos = mark
                raise
            if (l, c) in self.by:
                return self.by[(l, c)]
        raise _Bad


def decode(src, cap=NO_BOUND):
    """(status, output, src_used); src_used is None where it is unspecified (BAD_TOKEN, OUTPUT_CAPACITY)"""
    src = bytes(src)
    bits, out = _Bits(src), bytearray()

    def emit(chunk_len, fn):
        for i in range(chunk_len):
            if len(out) >= cap:
                raise _Full
            out.append(fn(i))

    try:
        while True:
            hdr = bits.get(3)                         # (the three header bits are needed together)
            final, btype = hdr & 1, hdr >> 1
            if btype == 3:
                raise _Bad
            if btype == 0:
                bits.pos = (bits.pos + 7) & ~7
                v = bits.get(32)
                n = v & 0xFFFF
                if (n ^ 0xFFFF) != v >> 16:
                    raise _Bad
                p = bits.pos >> 3
                have = min(n, len(src) - p)
                emit(have, lambda i: src[p + i])
                bits.pos += 8 * have
                if have < n:
                    raise _Trunc
            else:
                if btype == 1:
                    lit, dist = _Code(FIXED_LIT), _Code(FIXED_DIST)
                else:
                    v = bits.get(14)
                    nlen, ndist, ncl = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
                    if nlen > 286 or ndist > 30:
                        raise _Bad
                    cl_lens = [0] * 19
                    for i in range(ncl):
                        cl_lens[CL_ORDER[i]] = bits.get(3)
                    _check_set(cl_lens, True)
                    total = nlen + ndist
                    if not any(cl_lens):              # zlib reads every length as a 1-bit 0 and then misses symbol 256
                        if bits.left() < total:
                            raise _Trunc
                        raise _Bad
                    cl = _Code(cl_lens)
                    lens = []
                    while len(lens) < total:
                        mark = bits.pos
                        s = cl.read(bits)
                        if s < 16:
                            lens.append(s)
                            continue
                        try:
                            ev = bits.get((2, 3, 7)[s - 16])
                        except _Trunc:
                            bits.pos = mark
                            raise
                        if s == 16 and not lens:
                            raise _Bad
                        rep = (3, 3, 11)[s - 16] + ev
                        if len(lens) + rep > total:
                            raise _Bad
                        lens += [lens[-1] if s == 16 else 0] * rep
                    if lens[256] == 0:
                        raise _Bad
                    _check_set(lens[:nlen], False)
                    _check_set(lens[nlen:], False)
                    lit, dist = _Code(lens[:nlen]), _Code(lens[nlen:])
                while True:
                    mark = bits.pos
                    try:
                        s = lit.read(bits)
                        if s < 256:
                            emit(1, lambda i: s)
                            continue
                        if s == 256:
                            break
                        if s > 285:
                            raise _Bad
                        length = LEN_BASE[s - 257] + bits.get(LEN_EXTRA[s - 257])
                        d = dist.read(bits)
                        if d > 29:
                            raise _Bad
                        distance = DIST_BASE[d] + bits.get(DIST_EXTRA[d])
                    except _Trunc:
                        bits.pos = mark
                        raise
                    if distance > len(out):
                        raise _Bad
                    emit(length, lambda i: out[-distance])
            if final:
                return OK, bytes(out), (bits.pos + 7) >> 3
    except _Trunc:
        return TRUNC, bytes(out), len(src)
    except _Bad:
        return BAD, bytes(out), None
    except _Full:
        return CAPACITY, bytes(out), None
