"""Built streams for the token-queue decoders (alz_decode_queue_kernel / alz_decode_queue2_kernel): the chunked copy phase (csrc/alz_emit_chunk.h)
and the element walk of the parse rounds (lane_walk_pos and the *_parse_round functions of csrc/alz_decode_fast.h).  Pure Python, shared by
tests/test_chunk_phase_cpu.py (the oracle pins every stream) and tests/test_gpu_chunk_phase.py (the kernels decode them).

A builder returns [(name, tokens, extras)] for one format row; `tokens` is a token list of tests/test_gpu_scalar_paths.py, written out by the row's writer of
tests/token_bodies.py.  extras: `case_end` (index behind the last token a case is about: the tail rule is checked against it), `marks` (what the CPU file
re-derives: output positions, chunk counts, landing offsets), `residues` (run at every destination residue), `cap` and `status` (a status case),
`no_margin` (the tail rule is broken on purpose).

How a stream is laid out
  lead   fresh literals (random bytes, a 4-byte repeat every 50 so that every element stays small) up to the output position the case wants
  sync   an element the row's parse round REFUSES (SYNC below, the line of the round beside it).  The round in front of it ends at it, the exact parser
         takes that one element, and the next round starts at the byte behind it: what follows a sync is the FIRST element of a round, whatever the lead was.
         This is the model of a round start used here; it needs no knowledge of how far the filler rounds advance.  A row without a refused element
         (FastLZ level 1) gets the same token lists without that guarantee (NOT_EXPRESSIBLE says so).
  group  the case.  Its elements are matches of a few input bytes each, so a whole group starts inside the 256-byte window of its round and is ONE batch of the
         copy phase; a step is 64 chunks of it (a token of n bytes is ceil(n / 16) chunks -- ceil(n / d) for an overlapping match of distance d < 16 other
         than 1, 2, 4).  `chunks_of` restates that and the CPU file asserts the counts.
  tail   at least 1 200 input bytes of short elements: a round runs only with QCH + 76 input bytes ahead of it (QCH = 1024 for CNX2, 512 otherwise)

Input offsets are found by writing a prefix of the token list: for two prefixes that both end where an element ends, the difference of their sizes is the
input distance of the two places (every writer's terminator has a fixed size)."""
import functools

import numpy as np

import token_bodies as TB
from auroralib.compression_amd import _abi as A
from token_bodies import BREAK, LIT, MATCH

RING = 4096                       # ALZ_QUEUE_LW
FAR_LEAD = 4096 + 2560 + 400      # output position from which a full ring and a far source exist
TAIL_INPUT = 1200
QAHEAD_MAX = 1024 + 76


class Row:
    def __init__(self, name, min_len, max_len, sync, sync_cite, lit_max=200):
        self.name = name
        self.fmt, self.W, _, _, self.body, self.lz = TB.EDGE_FORMATS[name]
        self.min_len, self.max_len, self.sync, self.sync_cite, self.lit_max = min_len, max_len, sync, sync_cite, lit_max
        self.e2 = self.fmt not in TB.FIRST_IS_LITERAL
        # input bytes the reference leaves unread: LZShrek's reader takes the match flag and the length byte behind a last literal group as the end mark
        # (LZShrek.cs:96-108), two of the four zero bytes its writer appends (LZShrek.cs:121-174)
        self.unread = 2 if name == "lzshrek" else 0
        self._written = {}

    def write(self, tokens):
        toks = list(tokens)
        if self.fmt == A.FMT_LZ4_BLOCK and (not toks or toks[-1][0] == MATCH):
            toks += [(LIT, 7)] * 5                       # (a block ends in literals, LZ4.cs:202-238)
        return self.body(toks)

    def size(self, tokens):
        return len(self.write(tokens))

    def written(self, tokens, k=None):
        """write(tokens[:k]) of a token list that `cases` keeps alive, written once"""
        key = (id(tokens), len(tokens) if k is None else k)
        if key not in self._written:                     # (the entry holds the list, so its id cannot pass to another one)
            self._written[key] = (tokens, self.write(tokens if k is None else tokens[:k]))
        assert self._written[key][0] is tokens
        return self._written[key][1]


def _fresh(rng, k):
    return [(LIT, int(x)) for x in rng.integers(1, 256, k)]


# The element each row's round refuses, as tokens (rng -> list), and the line that refuses it.
def _sync_run(rng):
    return _fresh(rng, 201)


COPY_ROWS = [
    # LZ4: a literal run above ALZ_QRUN; the sequence's match is part of the refused element
    Row("lz4_block", 4, 100000, lambda rng: [(MATCH, 1500, 8)] + _fresh(rng, 201) + [(MATCH, 1500, 8)], "lz4_parse_round: L0 + lx > ALZ_QRUN, alz_decode_fast.h:638"),
    # LZO: a match whose length takes a second extension byte (289 bytes and more: _lzo_ext writes a 0 first); it ends in a match, so a literal run can follow it
    Row("lzo", 3, 100000, lambda rng: [(MATCH, 1500, 300)], "lzo_interpret_bytes: bad = ext && e1 == 0, alz_decode_fast.h:1263"),
    Row("snappy_raw", 4, 64, _sync_run, "snappy_parse_round: len > ALZ_QRUN, alz_decode_fast.h:734"),
    Row("fastlz", 3, 264, None, "fastlz_parse_round refuses level 2's chained length byte only, alz_decode_fast.h:1163", lit_max=32),
    Row("fastlz_level2", 3, 100000, lambda rng: [(MATCH, 1500, 300)], "fastlz_parse_round: l2 && ext && e1 == 255, alz_decode_fast.h:1163", lit_max=32),
    Row("wflz", 5, 255, lambda rng: [(MATCH, 1500, 8)] + _fresh(rng, 201), "wflz_parse_round: plain > ALZ_QRUN, alz_decode_fast.h:1023"),
    Row("wflz_be", 5, 255, lambda rng: [(MATCH, 1500, 8)] + _fresh(rng, 201), "wflz_parse_round: plain > ALZ_QRUN, alz_decode_fast.h:1023"),
    # RefPack: a literal run is at most 112 bytes, what the round refuses is distance 131 072 (E2 makes it expressible anywhere: it reads zeros)
    Row("refpack", 5, 1028, lambda rng: [(MATCH, 0x20000, 5)], "refpack_parse_round: distance > 0x1FFFF, alz_decode_fast.h:1086", lit_max=112),
    Row("hig", 4, 0xFFFF, lambda rng: [(MATCH, 1500, 8)] + _fresh(rng, 201), "hig_parse_round: cnt > ALZ_QRUN, alz_decode_fast.h:979"),
]
# the queue rows without read-back (whole window in LDS) and PRS: walk families only
WALK_ONLY_ROWS = [
    Row("cns", 3, 130, lambda rng: [(BREAK,)], "cns_parse_round: an empty literal run, b == 0, alz_decode_fast.h:1127", lit_max=127),
    Row("cnx2", 4, 35, None, "cnx2_parse_round refuses groups above 700 bytes only (alz_decode_fast.h:803)", lit_max=200),
    Row("lzshrek", 3, 262, lambda rng: _fresh(rng, 201), "lzshrek_parse_round: lits > ALZ_QRUN, alz_decode_fast.h:897"),
    Row("prs_be", 3, 256, None, "prs_lane_parse walks flag bytes, no element is refused by size", lit_max=1),
    Row("prs_le", 3, 256, None, "prs_lane_parse walks flag bytes, no element is refused by size", lit_max=1),
]
ROWS = {r.name: r for r in COPY_ROWS + WALK_ONLY_ROWS}
COPY_FAMILIES = ("C1", "C2", "C3", "C4", "C5", "C6", "C7", "C8", "C9", "C10")
WALK_FAMILIES = ("W1", "W2", "W3", "W4")

# (row, family, case) -> why the row's grammar has no such stream.  Nothing is left out silently: test_chunk_phase_cpu pins the count per row.
NOT_EXPRESSIBLE = {}


def _no(row, family, case, why):
    NOT_EXPRESSIBLE[(row.name, family, case)] = why


def expand(tokens):
    """test_gpu_scalar_paths.expand, by slices (the CPU file holds the two against each other): out[q] = out[q - d], zero in front of the stream start (E2)"""
    out, run = bytearray(), bytearray()
    for t in tokens:
        if t[0] == LIT:
            run.append(t[1])
            continue
        if t[0] == BREAK:
            continue
        if run:
            out += run; run = bytearray()
        d, n = t[1], t[2]
        while n:
            have = len(out)
            if d > have:                                 # E2
                k = min(n, d - have)
                out += bytes(k); n -= k
                continue
            k = min(n, d)
            out += out[have - d:have - d + k]; n -= k
    return bytes(out + run)


def chunks_of(d, n, run=False):
    """chunks of one token in emit_steps (alz_emit_chunk.h:327-333)"""
    if not run and d < 16 and d < n and d not in (1, 2, 4):
        return -(-n // d)
    return -(-n // 16)


class B:
    """a stream under construction: tokens, output position, marks"""

    def __init__(self, row, seed):
        self.row, self.rng, self.toks, self.pos, self.marks, self.case_end = row, np.random.default_rng(seed), [], 0, [], 0

    def lit(self, k):
        self.toks += _fresh(self.rng, k); self.pos += k
        return self

    def match(self, d, n):
        if d > self.row.W and self.row in WALK_ONLY_ROWS:   # (the small windows: the walk families' distances are folded into them)
            d = 20 + d % (self.row.W - 40)
        assert self.row.min_len <= n <= self.row.max_len and 1 <= d <= self.row.W, (self.row.name, d, n)
        assert d <= self.pos or self.row.e2, (self.row.name, d, self.pos)
        self.toks.append((MATCH, d, n)); self.pos += n
        return self

    def start(self):
        """the first elements: literals, so that every row's rounds have started (LZO ls.started, FastLZ fz.started, HIG s.bits != 0, queue2's s.p >= 4)"""
        self.lit(40).match(17, self.row.min_len).lit(12).match(23, self.row.min_len)
        return self

    def lead_to(self, P):
        assert P >= self.pos, (P, self.pos)
        while P - self.pos > 120:
            self.lit(50).match(int(self.rng.integers(20, 41)), self.row.min_len)
        return self.lit(P - self.pos)                    # (rows with short literal elements: the writer splits the run)

    def add(self, tokens):
        for t in tokens:
            if t[0] == BREAK:
                self.toks.append(t)
            elif t[0] == LIT:
                self.toks.append(t); self.pos += 1
            else:
                self.match(t[1], t[2])
        return self

    def sync(self):
        """-> True when the row has a refused element.  Its output length is SYNC_LEN[row]."""
        if self.row.sync is None:
            return False
        self.add(self.row.sync(self.rng))
        return True

    def sync_at(self, P):
        """a sync whose last byte is in front of output position P"""
        self.lead_to(P - sync_len(self.row))
        return self.sync()

    def full_step_less(self, k=1):
        """64 - k chunks of plain 48- and 16-byte matches from fresh, settled sources (near: inside the ring, in front of the step)"""
        c, i = 64 - k, 0
        while c:
            n = 48 if c >= 3 else 16 * c
            self.match(1100 + 13 * i, n); c -= n // 16; i += 1
        return self

    def mark(self, **kw):
        self.marks.append(dict(kw, pos=self.pos, tok=len(self.toks)))
        return self

    def end_case(self):
        self.case_end = len(self.toks)
        return self

    def tail(self, input_bytes=TAIL_INPUT, match_first=False):
        if match_first:
            self.match(int(self.rng.integers(30, 60)), self.row.min_len)
        for _ in range(-(-input_bytes // 21)):
            self.lit(20).match(int(self.rng.integers(30, 60)), self.row.min_len)
        self.lit(5)
        return self

    def done(self, name, **extras):
        return (name, self.toks, dict(extras, case_end=self.case_end, marks=self.marks))


@functools.lru_cache(maxsize=None)
def _sync_len(name):
    row = ROWS[name]
    if row.sync is None:
        return 0
    return sum(1 if t[0] == LIT else 0 if t[0] == BREAK else t[2] for t in row.sync(np.random.default_rng(0)))


def sync_len(row):
    return _sync_len(row.name)


def _lens(row, wanted):
    return sorted({n for n in wanted if row.min_len <= n <= row.max_len})


def _seed(row, family, k=0):
    return [row.fmt, {"fastlz_level2": 1}.get(row.name, 0), int(family[1:]) + (100 if family[0] == "W" else 0), k]


# ------------------------------------------------------------------------------------------------ copy families
C1_DIST = (2559, 2560, 2561, 2562, 3583, 3584, 4095, 4096, 4097, 4096 + 2560)
C1_LEN = (15, 16, 17, 20, 33)


def c1(row):
    """Ring / read-back line (alz_emit_chunk.h:224): the match as the first chunk of a step, and as the last chunk of a step whose 64 chunks give the full 1 KiB."""
    out = []
    if row.sync is None:
        _no(row, "C1", "placement in the step", "no refused element, the match's place in its step is by chance: " + row.sync_cite)
    for d in C1_DIST:
        for last in (False, True):
            b = B(row, _seed(row, "C1", d * 2 + last)).start().lead_to(FAR_LEAD)
            for n in _lens(row, (row.min_len,) + C1_LEN):
                b.sync()
                if last:
                    b.full_step_less(1)
                b.mark(d=d, n=n, chunk=63 if last else 0).match(d, n).lit(24)
            out.append(b.end_case().tail().done("C1 d=%d %s" % (d, "last chunk of a full step" if last else "first chunk")))
    return out


def c2(row):
    """Alignment: distances 2560, 2561, 4097, length 20, 0..3 literals in front of the match, both placements; the GPU file runs every stream at the sixteen
    destination residues (extras['residues'])."""
    out = []
    for d in (2560, 2561, 4097):
        for last in (False, True):
            b = B(row, _seed(row, "C2", d * 2 + last)).start().lead_to(FAR_LEAD)
            for phase in range(4):
                b.sync()
                if last:
                    b.full_step_less(2 if phase else 1)      # (the literals in front are a chunk of their own)
                if phase:
                    b.lit(phase)
                b.mark(d=d, n=20, phase=phase).match(d, 20).lit(24 + phase)
            out.append(b.end_case().tail().done("C2 d=%d %s" % (d, "last" if last else "first"), residues=True))
    return out


C3_DIST = (2600, 2601, 2602, 2603)


def c3(row):
    """Far source at the stream start: the 20-byte read-back of a chunk starts at position fp = p - d - b, b = p & 3 (alz_emit_chunk.h:241-252), and the byte-wise
    path decides per byte whether it lies in front of position 0 (:249).  p - d over 0 .. 6 at four distances of every residue mod 4 gives fp every value of
    -3 .. +3 (the CPU file asserts the set per row; b is (p + oshift) & 3 in the kernel and the streams' destinations are 16-aligned here -- at another
    residue the four distance residues still give the whole set) with the source itself inside the stream, so the rows without E2 enter that path too; for the rows whose
    streams may start with a match also p - d = -3 .. -1 and the distances p + 1, p + 17 and W (E2: zeros)."""
    out = []
    for d in C3_DIST:
        for delta in range(-3 if row.e2 else 0, 7):
            for n in _lens(row, (row.min_len, 20)) if d != 2600 else _lens(row, (row.min_len, 16, 20, 33)):
                p = d + delta
                b = B(row, _seed(row, "C3", ((d - 2600) * 16 + delta + 8) * 64 + n)).start().lead_to(p)
                b.mark(d=d, n=n, fp=p - d - (p & 3)).match(d, n).lit(24)
                out.append(b.end_case().tail().done("C3 d=%d p - d = %d n=%d" % (d, delta, n)))
    if not row.e2:
        _no(row, "C3", "source in front of position 0", "no stream of this format starts with a match (token_bodies.FIRST_IS_LITERAL: WFLZ.cs:130-159, FastLZ.cs:181-198, LZO.cs:59-64)")
        return out
    p = 2700
    for d in (p + 1, p + 17, row.W):
        b = B(row, _seed(row, "C3", d)).start().lead_to(p)
        b.mark(d=d, n=20).match(d, 20).lit(24)
        out.append(b.end_case().tail().done("C3 E2 d=%d at %d" % (d, p)))
    return out


C4_DIST = tuple(range(1, 34)) + (63, 64, 65)


def _c4_lens(row, d):
    return _lens(row, (d - 1, d, d + 1, 2 * d + 1, 15, 16, 17, 31, 32, 33, 47, 100, 1023, 1024))


def c4(row):
    """Self-overlap: register replication (d = 1, 2, 4), d-byte chunks (other d < 16), the pattern in front through umod24 (larger d); in mid-ring and ending 5
    bytes past a multiple of 4096."""
    out = []
    for d in C4_DIST:
        lens = _c4_lens(row, d)
        b = B(row, _seed(row, "C4", d)).start().lead_to(RING + 300)
        for n in lens:
            b.mark(d=d, n=n).match(d, n).lit(19)
        out.append(b.end_case().tail().done("C4 d=%d mid-ring" % d))
        for i in range(0, len(lens), 3):
            b = B(row, _seed(row, "C4", 1000 + d * 16 + i)).start()
            for k, n in enumerate(lens[i:i + 3]):
                b.lead_to(RING * (k + 1 + (1 if n > 900 else 0)) + 5 - n)
                b.mark(d=d, n=n, ends=5).match(d, n).lit(19)
            out.append(b.end_case().tail().done("C4 d=%d ending 5 past the seam, lengths %r" % (d, lens[i:i + 3])))
    for n in (1023, 1024):
        if n > row.max_len:
            _no(row, "C4", "length %d" % n, "the longest match of this row is %d bytes (token_bodies.EDGE_FORMATS)" % row.max_len)
    return out


C5_LEN = (1025, 2047, 2048, 2049, 3000, 5000)
C5_DIST = (1, 2, 3, 4, 5, 7, 15, 16, 17, 100, 1023, 1024, 1025, 2560, 2561, 3000, 4097)


def c5(row):
    """Tokens above ALZ_LONGTOK run alone, sources folded (LATER, alz_emit_chunk.h:211-215); distances 2561, 3000, 4097: far, long and overlapping at once."""
    lens = _lens(row, C5_LEN)
    if not lens:
        _no(row, "C5", "all", "the longest match of this row is %d bytes (token_bodies.EDGE_FORMATS): no token above ALZ_LONGTOK" % row.max_len)
        return []
    for n in C5_LEN:
        if n not in lens:
            _no(row, "C5", "length %d" % n, "the longest match of this row is %d bytes (RefPack.cs:241-303)" % row.max_len)
    out = []
    for d in C5_DIST:
        for i in range(0, len(lens), 3):
            b = B(row, _seed(row, "C5", d * 8 + i)).start().lead_to(RING + 300)
            for n in lens[i:i + 3]:
                b.mark(d=d, n=n).match(d, n).lit(21)
            out.append(b.end_case().tail().done("C5 d=%d lengths %r" % (d, lens[i:i + 3])))
    b = B(row, _seed(row, "C5", 9999)).start().lead_to(RING + 300)
    for d in (3, 100, 2561):
        b.mark(d=d, n=lens[0], dependent=True).match(d, lens[0]).match(5, 9).match(lens[0] + 9, 20).lit(21)
    out.append(b.end_case().tail().done("C5 a short dependent match directly behind the long token"))
    return out


def c6(row):
    """Dependency chains inside one step: n fresh bytes, then k matches of distance n and length n, each copying the token in front of it (depth >= 2: `shallow`
    must be false, alz_emit_chunk.h:274-294); and a chain whose links alternate near (in-step) and far sources."""
    out = []
    for n in (4, 8, 16, 24):
        if n < row.min_len:
            _no(row, "C6", "n = %d" % n, "the shortest match of this row is %d bytes (token_bodies.EDGE_FORMATS)" % row.min_len)
            continue
        b = B(row, _seed(row, "C6", n)).start().lead_to(FAR_LEAD)
        for k in (1, 2, 3, 8, 40):
            b.sync()
            b.lit(n).mark(n=n, k=k)
            for _ in range(k):
                b.match(n, n)
            b.lit(24)
        b.sync()
        b.lit(16).mark(alternating=True)
        for far in (3000, 2600, 4097, 2561):
            b.match(16, 16).match(far, 16).match(16, 16)
        b.lit(24)
        out.append(b.end_case().tail().done("C6 n=%d" % n))
    return out


C7_OFF = (-20, -17, -16, -4, -1, 0, 1, 3, 4, 15, 16, 31, 32, 33)


def c7(row):
    """Ring seam and mirror (chunk_mirror, alz_emit_chunk.h:158): the DESTINATION, or the 24-byte aligned read of the SOURCE, starts at ring offset
    4096 k + off; each also directly behind a refused element, whose byte-wise writer has set slack_dirty."""
    out = []
    if row.sync is None:
        _no(row, "C7", "behind a refused element", "no refused element: " + row.sync_cite)
    for off in C7_OFF:
        for source in (False, True):
            for dirty in ((False, True, "ext2") if row.name == "lz4_block" else (False, True) if row.sync else (False,)):
                for pair in ((5, 16), (17, 20)):
                    b = B(row, _seed(row, "C7", (off + 32) * 32 + source * 16 + (2 if dirty == "ext2" else int(dirty)) * 4 + pair[0] % 3)).start()
                    for k, n in enumerate(_lens(row, pair)):
                        q = RING * (k + 1) + off + (1000 if source else 0)
                        if dirty == "ext2":              # an LZ4 sequence whose literal length takes a second extension byte (lz4_parse_round:638, e1 == 255)
                            b.lead_to(q - 286).match(1500, 8).lit(270).match(1500, 8)
                        elif dirty:
                            b.sync_at(q)
                        else:
                            b.lead_to(q)
                        b.mark(n=n, off=off, source=source, d=1000 if source else 300).match(1000 if source else 300, n).lit(24)
                    out.append(b.end_case().tail().done("C7 %s at %d%s lengths %r" % ("source" if source else "destination", off, ", behind a sequence with a second extension byte" if dirty == "ext2" else ", behind a refused element" if dirty else "", pair)))
    return out


def c8(row):
    """Step composition (alz_emit_chunk.h:344-361): batches of 63 .. 129 chunks, a 5-chunk token across the step boundary at every split, 64 one-chunk tokens,
    d-byte chunks mixed with 16-byte ones."""
    out = []
    big = min(64, row.max_len // 16 * 16)
    b = B(row, _seed(row, "C8", 0)).start().lead_to(FAR_LEAD)
    for count in (63, 64, 65, 127, 128, 129):
        b.sync()
        b.mark(chunks=count)
        c, i = count, 0
        while c:
            n = min(big, 16 * c)
            b.match(1100 + 13 * i, n); c -= n // 16; i += 1
        b.mark(end=True).lit(24)
    out.append(b.end_case().tail().done("C8 batches of 63 .. 129 chunks"))
    if row.max_len >= 80:
        b = B(row, _seed(row, "C8", 1)).start().lead_to(FAR_LEAD)
        for first in (1, 2, 3, 4):
            b.sync()
            b.full_step_less(first)
            b.mark(split=(first, 5 - first)).match(700, 80).match(1300, 48).lit(24)
        out.append(b.end_case().tail().done("C8 a 5-chunk token across the step boundary"))
    else:
        _no(row, "C8", "5-chunk token", "the longest match of this row is %d bytes: four chunks (Snappy.cs:124-203)" % row.max_len)
    b = B(row, _seed(row, "C8", 2)).start().lead_to(FAR_LEAD)
    b.sync()
    b.mark(one_chunk_tokens=64)
    for i in range(32):
        b.lit(1).match(1100 + 13 * i, 16)
    b.mark(end=True).lit(24)
    out.append(b.end_case().tail().done("C8 64 one-chunk tokens"))
    n = min(1000, row.max_len)
    b = B(row, _seed(row, "C8", 3)).start().lead_to(FAR_LEAD)
    b.sync()
    b.mark(tsm=chunks_of(3, n)).match(1200, 16).match(1300, 16).match(3, n).match(1400, 16).match(7, min(n, 300)).match(1500, 16).lit(24)
    out.append(b.end_case().tail().done("C8 d-byte chunks (d = 3, %d bytes) mixed with 16-byte ones" % n))
    return out


def c9(row):
    """Literal runs (LITRUN): lengths at both sides of a chunk and of ALZ_QRUN, and runs of 1 024 / 1 025 bytes through the exact parser."""
    out = []
    if row.lit_max < 200:
        _no(row, "C9", "one element per run", "a literal element of this row holds at most %d bytes: longer runs are several elements" % row.lit_max)
    b = B(row, _seed(row, "C9", 0)).start().lead_to(RING + 300)
    for n in (1, 15, 16, 17, 199, 200, 201, 1024, 1025):
        b.mark(run=n).lit(n).match(500, 8)
    out.append(b.end_case().tail().done("C9 runs of 1 .. 1025"))
    for shift in range(8):                               # the same runs at other input phases
        b = B(row, _seed(row, "C9", 1 + shift)).start().lead_to(RING + 300 + shift)
        for n in (200, 199, 17, 200):
            b.mark(run=n).lit(n).match(500, 8)
        out.append(b.end_case().tail().done("C9 runs at input phase %d" % shift))
    # the largest run a round takes, its first byte at the last byte of a 512-byte input-cache chunk and two bytes to either side (the cache holds chunks of
    # the stream's input from offset 0 on: InCache, QCH = 512).  The run's offset is FOUND in the written body -- its bytes are random --, the lead is padded to move it
    n = min(200, row.lit_max)
    for want in (509, 510, 511, 512, 513):
        pad = 0
        for _ in range(12):
            b = B(row, _seed(row, "C9", 100 + want)).start().lead_to(RING + 300).match(500, 8).lit(pad).match(500, 8)
            b.mark(run=n, edge=want).lit(n).match(500, 8).lit(20)
            off = run_offset(row, b.toks, b.marks[-1])
            if off % 512 == want % 512:
                break
            pad = (pad + want - off) % 512
        assert off % 512 == want % 512, (row.name, want, off)
        out.append(b.end_case().tail().done("C9 a run of %d starts at input byte %d of a cache chunk" % (n, want)))
    b = B(row, _seed(row, "C9", 200)).start().lead_to(RING + 300).match(500, 8)
    b.mark(run=n, last=True).lit(n)
    out.append(b.end_case().tail(match_first=True).done("C9 a run of %d ends at the last input byte in front of the tail" % n))
    return out


def run_offset(row, tokens, mark):
    """input offset of the first byte of the literal run that stands at the mark, found in the written body"""
    run = bytes(t[1] for t in tokens[mark["tok"]:mark["tok"] + min(mark["run"], 24)])
    body = row.write(tokens)
    off = body.find(run)
    assert off >= 0 and body.find(run, off + 1) < 0
    return off


C10_ROWS = ("lz4_block", "wflz")


def c10(row):
    """Capacity cut (E5): one sequence of about 300 bytes behind a 7 KiB lead, dst_cap at every byte of it.  Status cases: the oracle is the reference."""
    if row.name not in C10_ROWS:
        return []
    b = B(row, _seed(row, "C10", 0)).start().lead_to(7168)
    b.sync()
    b.full_step_less(6)                                  # 58 chunks: the d = 3 match below crosses the step
    lo = b.pos
    b.lit(30).match(3000, 40).lit(9).match(3, 100).lit(17).match(60, 33).lit(11).match(2561, 20).lit(40)
    hi = b.pos
    name, toks, ex = b.end_case().tail().done("C10")
    return [("C10 cap=%d" % cap, toks, dict(ex, cap=cap, status=A.ST_OUTPUT_CAPACITY)) for cap in range(lo, hi + 1)]


# ------------------------------------------------------------------------------------------------ walk families
LIT_CITE = {A.FMT_FASTLZ: "FastLZ.cs:63-160", A.FMT_REFPACK: "RefPack.cs:177-245", A.FMT_CNS: "CNS.cs:83-106"}
W1_TARGETS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 255)


LITS_FIRST = ("lz4_block", "snappy_raw", "lzo", "fastlz", "fastlz_level2", "refpack", "cns", "lzshrek")     # an element's literals stand in front of its match (or alone)


def _w1_prefix(row, seed):
    b = B(row, seed).start().lead_to(1700)
    b.sync()
    return b


def landing(row, tokens, mark):
    """input offset of the element that starts at token mark['tok'], relative to the round start (the byte behind the sync, token mark['round'])"""
    return row.size(tokens[:mark["tok"]]) - row.size(tokens[:mark["round"]])


@functools.lru_cache(maxsize=None)
def _fill_sizes(name):
    row = ROWS[name]
    big = min(10, row.lit_max)
    base = _filled(row, [big], 0, 0)
    sizes = []                                           # input bytes of "r literals and a shortest match" as a filler element
    for r in range(big + 1):
        b = _filled(row, [big, r], 0, 0)
        sizes.append(landing(row, b.toks, b.marks[-1]) - landing(row, base.toks, base.marks[-1]))
    return big, sizes, landing(row, base.toks, base.marks[-1]) - sizes[big]


def _filled(row, fill, tgt, seed):
    """behind a sync: the round's first element (a bare match), then one filler element per entry of `fill` (that many literals and a shortest match); the mark
    stands where the next element starts"""
    b = _w1_prefix(row, _seed(row, "W1", seed))
    rnd = len(b.toks)
    b.match(310, row.min_len)                            # (a filler's literals must not join the refused run)
    for r in fill:
        b.lit(r).match(300, row.min_len)
    b.marks.append(dict(tok=len(b.toks), round=rnd, target=tgt, pos=b.pos))
    return b


def placed_at(row, tgt, seed):
    """a builder whose next element starts at byte `tgt` of its round's window, or None"""
    big, sizes, first = _fill_sizes(row.name)
    for a, r1, r2 in ((a, r1, r2) for a in range(31) for r1 in range(big + 1) for r2 in range(big + 1)):
        if first + a * sizes[big] + sizes[r1] + sizes[r2] != tgt:
            continue
        b = _filled(row, [big] * a + [r1, r2], tgt, seed)
        if landing(row, b.toks, b.marks[-1]) == tgt:     # (the sum is a guess -- LZO's short runs ride in the match in front --, the written prefix decides)
            return b
    return None


def walk_model(sizes):
    """lane_walk_pos restated for a list of element sizes (alz_decode_fast.h:566-599): a window of 64 bytes is entered while fewer than 33 elements are taken and
    the offset lies in front of its end; -> the offset of every element inside its round"""
    out, i = [], 0
    while i < len(sizes):
        sp, cnt = 0, 0
        for w in range(4):
            if cnt < 33 and sp < 64 * (w + 1):
                while sp < 64 * (w + 1) and i < len(sizes):
                    out.append(sp); sp += sizes[i]; i += 1; cnt += 1
    return out


def model_sizes(row, tokens, mark):
    """element sizes from the model's origin (the byte behind the stream's first elements) to the mark: a literal run of r bytes is an element of r + 1, a match
    one of `m` bytes (one token per element: FastLZ.cs:63-160, CNS.cs:77-108)"""
    sizes, run = [], 0
    for t in tokens[mark["origin"]:mark["tok"]]:
        if t[0] == LIT:
            run += 1
            continue
        if run:
            sizes.append(run + 1); run = 0
        sizes.append(mark["m"])
    assert run == 0
    return sizes


def _w1_filler_model(row):
    """Rows without a refused element: the stream is filler of one element size from its first elements on, so a round starts at every multiple of the
    filler's round advance (walk_model restates `adv` of such a round; the origin is modelled as the byte behind the first elements, which the exact parser
    takes).  One literal element in front shifts the phase."""
    out = []
    b0 = B(row, 0).start()
    m = row.size(b0.toks + [(MATCH, 30, row.min_len)] * 2) - row.size(b0.toks + [(MATCH, 30, row.min_len)])
    for tgt in W1_TARGETS:
        found = None
        for F, r, K in ((F, r, K) for F in (0, 8, 14, 20) for r in range(0, 24) for K in range(0, 130)):
            if F and (K == 0 or F + r > row.lit_max):
                continue
            sizes = ([F + r + 1, m] + [F + 1, m] * (K - 1)) if F else ([r + 1] if r else []) + [m] * K     # (the phase literals join the first filler run)
            if sum(sizes) >= tgt and walk_model(sizes + [m])[-1] == tgt:
                found = (F, r, K); break
        if found is None:
            _no(row, "W1", "byte %d" % tgt, "walk_model finds no filler of literal elements and matches of %d bytes that lands there" % m)
            continue
        F, r, K = found
        b = B(row, _seed(row, "W1", tgt)).start()
        origin = len(b.toks)
        b.lit(r)
        for i in range(K):
            b.lit(F).match(30 + i % 20, row.min_len)
        b.marks.append(dict(tok=len(b.toks), origin=origin, m=m, model_target=tgt, pos=b.pos))
        b.match(50, 9).lit(20)
        out.append(b.end_case().tail().done("W1 (filler model) an element starts at byte %d" % tgt))
    for jump in (70, 130):
        if jump > row.lit_max:
            _no(row, "W1", "an element of %d bytes" % jump, "a literal element of this row holds at most %d bytes (%s)" % (row.lit_max, LIT_CITE[row.fmt]))
            continue
        b = B(row, _seed(row, "W1", 1000 + jump)).start()
        b.match(30, row.min_len).lit(jump).match(40, 9).lit(jump).match(50, 9).lit(20)
        out.append(b.end_case().tail().done("W1 an element of %d bytes jumps sub-windows" % jump))
    return out


def _w1_flag_sweep(row):
    """CNX2 and PRS walk flag bytes (a flag byte and the tokens its bits announce are the unit, cnx2_parse_round / prs_lane_parse): the same tokens behind 0 .. 63
    literals, so that every flag byte of the stream takes every position mod 64 of its window.  A sweep, not a placement."""
    out = []
    for phase in range(64):
        b = B(row, _seed(row, "W1", phase)).start().lit(phase)
        b.mark(sweep=phase)
        for i in range(60):
            b.match(30 + i, row.min_len + i % 3).lit(i % 6)
        b.match(40, 9).lit(20)
        out.append(b.end_case().tail().done("W1 flag bytes at phase %d" % phase))
    return out


def w1(row):
    """Landing: an element (a bare match behind a match) starts at byte 63 .. 255 of the round's 256-byte window; the largest element a round takes starts at
    byte 255; elements that jump one and two sub-windows."""
    if row.name in ("cnx2", "prs_be", "prs_le"):
        return _w1_flag_sweep(row)
    if row.sync is None:
        return _w1_filler_model(row)
    out = _w1_filler_model(row) if row.name == "cns" else []
    # LZShrek: up to eight matches share one group header, so only an element that STARTS a group -- one with literals -- is sure to start where the written
    # prefix ends (LZShrek.cs:84-94): its landing element is three literals and a match
    head = 3 if row.name == "lzshrek" else 0
    R = min(200, row.lit_max)
    for tgt in W1_TARGETS:
        b = placed_at(row, tgt, tgt)
        if b is None:
            _no(row, "W1", "byte %d" % tgt, "no sequence of at most 32 elements of this grammar ends exactly there")
            continue
        b.lit(head).match(400, 9).match(500, 9).lit(20)
        out.append(b.end_case().tail().done("W1 an element starts at byte %d" % tgt))
        if tgt == 255:                                   # the largest element a round takes starts there: R literals and a match, in the row's order
            b = placed_at(row, tgt, tgt)
            b.marks[-1]["reach"] = R
            if row.name in LITS_FIRST:
                b.lit(R).match(400, 9)
            else:
                b.match(400, 9).lit(R)
            b.match(500, 9).lit(20)
            out.append(b.end_case().tail().done("W1 the element at byte 255 holds %d literals" % R))
    for jump in (70, 130):
        if jump > row.lit_max:
            _no(row, "W1", "an element of %d bytes" % jump, "a literal element of this row holds at most %d bytes (%s)" % (row.lit_max, LIT_CITE[row.fmt]))
            continue
        b = _w1_prefix(row, _seed(row, "W1", 1000 + jump))
        b.match(300, row.min_len).lit(jump).match(400, 9).lit(jump).match(500, 9).lit(20)
        out.append(b.end_case().tail().done("W1 an element of %d bytes jumps sub-windows" % jump))
    return out


def w2(row):
    """Counts: minimum-size elements only, so that a round meets more elements (and more tokens) than 64 lanes hold; token totals 63 / 64 / 65 over the
    candidate elements with 31 / 32 / 33 of them carrying a literal (lz4_parse_round:660-663 and its siblings)."""
    out = []
    for lits in (0, 1):
        b = B(row, _seed(row, "W2", lits)).start().lead_to(1700)
        b.sync()
        b.mark(min_elements=200)
        for i in range(200):
            if lits:
                b.lit(1)
            b.match(100 + 3 * (i % 50), row.min_len)
        out.append(b.end_case().tail().done("W2 200 shortest elements, %d literal each" % lits))
    for total in (63, 64, 65):
        for carrying in (31, 32, 33):
            b = B(row, _seed(row, "W2", total * 64 + carrying)).start().lead_to(1700)
            b.sync()
            seqs = total - carrying
            b.mark(tokens=total, carrying=carrying)
            for i in range(seqs):
                if i < carrying:
                    b.lit(1)
                b.match(100 + 3 * i, row.min_len)
            for i in range(40):
                b.match(200 + i, row.min_len + 1)
            out.append(b.end_case().tail().done("W2 %d tokens over %d elements, %d carry a literal" % (total, seqs, min(carrying, seqs))))
    return out


def _form(tokens_of):
    return lambda rng: tokens_of(rng)


def _refused_forms(row):
    """(name, tokens(rng), line) of every element form the row's round refuses -- LZ4 and Snappy: also the forms next to them, which it takes"""
    n = row.name
    if n == "lz4_block":
        forms = [("L=%d" % L, (lambda L: lambda rng: _fresh(rng, L) + [(MATCH, 700, 8)])(L), "lz4_parse_round:638") for L in (14, 15, 200, 201, 269, 270)]
        return forms + [("M=%d" % M, (lambda M: lambda rng: [(MATCH, 700, M)])(M), "lz4_parse_round:638") for M in (18, 19, 273, 274)]
    if n == "snappy_raw":
        forms = [("literal of %d" % L, (lambda L: lambda rng: _fresh(rng, L))(L), "snappy_parse_round:734") for L in (60, 61, 200, 201, 256, 257)]
        return forms + [("copy with a 4-byte offset of 3000", lambda rng: [(MATCH, 3000, 12, "copy4")], "snappy_parse_round:736")]
    if n == "lzo":
        return [("run of 201", _sync_run, "lzo_interpret_bytes:1283 len > ALZ_QRUN"), ("run of 280 (extension byte 0)", lambda rng: _fresh(rng, 280), "lzo_interpret_bytes:1283 ext && e1 == 0"),
                ("match of 300 (second extension byte)", row.sync, "lzo_interpret_bytes:1263 bad = ext && e1 == 0")]
    if n == "hig":
        return [("201 literals behind a match", row.sync, "hig_parse_round:979 cnt > ALZ_QRUN"),
                ("match of 16 400", lambda rng: [(MATCH, 3, 16400)], "hig_parse_round:979 length > ALZ_TOK_MAXLEN")]
    if n == "cnx2":
        return [("group of four 255-byte runs", lambda rng: _fresh(rng, 1020), "cnx2_parse_round:803 off > 700")]
    if row.sync is None:
        return []
    return [("refused", row.sync, row.sync_cite)]


def w3(row):
    """Refused elements: the first one as the 1st (window byte 0), 2nd and 32nd element of what would be its round, at window bytes 63 and 64, and two back to
    back.  Every form is a stream of its own.  CNX2 has no second refused form to place the first by: its group stands behind 0 .. 3 tokens of a flag byte."""
    forms = _refused_forms(row)
    if not forms:
        _no(row, "W3", "all", "no refused element: " + row.sync_cite)
        return []
    if row.name == "refpack":
        _no(row, "W3", "b >= 0xFC (refpack_parse_round:1072)", "the stop code: it ends the stream, nothing stands behind it (RefPack.cs:177-245)")
    if row.name in ("wflz", "wflz_be"):
        _no(row, "W3", "(length | plain) == 0 (wflz_parse_round:1023)", "the end block: it ends the stream (WFLZ.cs:130-159)")
    if row.name == "lzshrek":
        _no(row, "W3", "lenb && e1 == 0 (lzshrek_parse_round:901)", "the end mark: it ends the stream (LZShrek.cs:96-108)")
    out = []

    def put(b, form, what):
        toks = form(b.rng)
        if b.toks[-1][0] == LIT and toks[0][0] == LIT and row.name == "snappy_raw":
            b.toks.append((BREAK,))                      # two literal elements side by side
        elif b.toks[-1][0] == LIT and toks[0][0] == LIT:
            _no(row, "W3", what, "two literal runs cannot stand side by side: behind a run an opcode below 16 is a match (LZO.cs:55), a group is one run and at least one match (LZShrek.cs:84-94), "
                "a block is one match field and one run (WFLZ.cs:130-159)")
            b.match(333, row.min_len)
        b.add(toks)

    for k, (fname, form, cite) in enumerate(forms):
        if row.sync is None:                             # CNX2
            for tgt in (63, 64):
                _no(row, "W3", "%s at window byte %d" % (fname, tgt), "the round refuses nothing else (cnx2_parse_round:803), so no round start is known to count window bytes from; "
                    "and four runs that share one flag byte start where the flag byte in front ends (CNX2.cs:83-139)")
            b = B(row, _seed(row, "W3", k)).start().lead_to(1700)
            for phase in range(4):
                for i in range(phase + 1):
                    b.match(100 + 3 * i, row.min_len)
                b.mark(form=fname, phase=phase, cite=cite)
                b.add(form(b.rng))
                b.match(450, 9).lit(20)
            out.append(b.end_case().tail().done("W3 %s" % fname))
            continue
        b = B(row, _seed(row, "W3", k)).start().lead_to(1700)
        long_form = fname == "match of 16 400"            # (one placement per stream: streams stay below 24 KiB)
        for before in (0,) if long_form else (0, 1, 31):
            b.sync()
            for i in range(before):
                b.match(100 + 3 * i, row.min_len)
            b.mark(form=fname, before=before, cite=cite)
            put(b, form, "%s as element 1 of a round" % fname)
            b.match(450, 9).lit(20)
        if not long_form:
            b.sync()
            b.match(444, row.min_len).mark(form=fname, back_to_back=True, cite=cite)
            put(b, form, fname)
            put(b, form, "%s twice back to back" % fname)
            b.match(450, 9).lit(20)
        out.append(b.end_case().tail().done("W3 %s" % fname))
        for tgt in (63, 64):
            b = placed_at(row, tgt, 5000 + 64 * k + tgt)
            if b is not None and row.name == "lzshrek" and form(np.random.default_rng(0))[0][0] != LIT:
                b = None
            if b is None:
                _no(row, "W3", "%s at window byte %d" % (fname, tgt), "no sequence of at most 32 elements of this grammar ends exactly there")
                continue
            b.marks[-1].update(form=fname, cite=cite)
            b.add(form(b.rng))
            b.match(450, 9).lit(20)
            out.append(b.end_case().tail().done("W3 %s at window byte %d" % (fname, tgt)))
    if row.name == "lzshrek":                            # a distance field beyond the 4 KiB window is a bad token (lzshrek_parse_round:901 dist > 0x1000; status case)
        for before in (0, 1, 31):
            b = B(row, _seed(row, "W3", 90 + before)).start().lead_to(6000)
            b.sync()
            for i in range(before):
                b.match(100 + 3 * i, row.min_len)
            b.mark(form="match at distance 5000", before=before, cite="lzshrek_parse_round:901")
            b.toks.append((MATCH, 5000, 9)); b.pos += 9
            b.match(450, 9).lit(20)
            out.append(b.end_case().tail().done("W3 distance 5000 behind %d elements of a round" % before, status=A.ST_BAD_TOKEN))
    if row.name == "snappy_raw":                         # E3: a 4-byte offset beyond the window is a bad token (status case)
        b = B(row, _seed(row, "W3", 99)).start().lead_to(1700)
        b.sync()
        b.match(300, 8).mark(form="copy with a 4-byte offset of 70 000", cite="snappy_parse_round:736")
        b.toks.append((MATCH, 70000, 12, "copy4")); b.pos += 12
        b.match(450, 9).lit(20)
        out.append(b.end_case().tail().done("W3 copy with a 4-byte offset beyond 65 536", status=A.ST_BAD_TOKEN))
    return out


def w4(row):
    """Input margin: one W1 landing case (an element at window byte 128; the rows without a placed round: 30 short elements), the trailing filler tuned so that
    exactly QCH + 76 + 16 k input bytes lie behind the case, k = -6 .. 6, for QCH = 512 and 1024: the switch to the exact parser (s.p + QAHEAD > src_len)
    falls before, inside and behind the case.  These streams break the tail rule on purpose (no_margin)."""
    out = []
    for around in (512 + 76, 1024 + 76):
        for k in range(-6, 7):
            want, budget = around + 16 * k, around + 16 * k
            for _ in range(8):
                b = placed_at(row, 128, 7000) if row.sync is not None and row.name != "lzshrek" else None
                if b is None:
                    b = B(row, _seed(row, "W4", 0)).start().lead_to(1700)
                    b.sync()
                    for i in range(30):
                        b.lit(i % 3).match(100 + 3 * i, row.min_len)
                b.match(3, min(60, row.max_len)).match(400, 9)
                b.end_case()
                left = budget
                while left > 0:
                    r = min(left, 20)
                    b.lit(r); left -= r + 3
                    if left > 0:
                        b.match(40, row.min_len)
                b.lit(5)
                behind = row.size(b.toks) - row.size(b.toks[:b.case_end])
                if behind == want:
                    break
                budget += want - behind
            b.marks.append(dict(tail_input=want, behind=behind, tok=len(b.toks), pos=b.pos))
            out.append(b.done("W4 %d input bytes behind the case" % behind, no_margin=True))
    return out


FAMILIES = dict(C1=c1, C2=c2, C3=c3, C4=c4, C5=c5, C6=c6, C7=c7, C8=c8, C9=c9, C10=c10, W1=w1, W2=w2, W3=w3, W4=w4)


@functools.lru_cache(maxsize=None)
def cases(row_name, family):
    """[(name, tokens, extras)] -- built once, shared, never changed"""
    row = ROWS[row_name]
    if family[0] == "C" and row not in COPY_ROWS:
        return ()
    return tuple(FAMILIES[family](row))


def has_cases(row_name, family):
    """whether (row, family) has streams at all, without building them (the CPU file holds this against `cases`)"""
    row = ROWS[row_name]
    if family[0] == "C":
        return row in COPY_ROWS and (family != "C10" or row_name in C10_ROWS) and (family != "C5" or row.max_len > 1024)
    return family != "W3" or bool(_refused_forms(row))


def build_all():
    """every builder run once, in one order: NOT_EXPRESSIBLE is complete and the same whoever asks"""
    for row_name in ROWS:
        for family in families_of(row_name):
            cases(row_name, family)
    return NOT_EXPRESSIBLE


def families_of(row_name):
    return (COPY_FAMILIES if ROWS[row_name] in COPY_ROWS else ()) + WALK_FAMILIES


def item(row, tokens, extras, want):
    """the dict tests/gpu_common.pack_streams takes"""
    it = dict(fmt=row.fmt, src=row.written(tokens))
    cap = extras.get("cap", len(want))
    sized = row.fmt not in (A.FMT_LZ4_BLOCK, A.FMT_SNAPPY_RAW, A.FMT_PRS_BE, A.FMT_PRS_LE, A.FMT_LZO)      # (test_gpu_big_stream.ELEM: no size in the descriptor)
    status = extras.get("status")
    it.update(decom_len=len(want) if sized else 0, cap=cap, want=want if status is None else None, cut=status is not None, what=None)
    return it
