"""The distance and length limits of every format of the main codec, and inputs that stand exactly on them.  TEST-ONLY; shared by
tests/test_geometry_edges_cpu.py (the inputs prove themselves against the oracle and the finder restatement) and tests/test_gpu_geometry_edges.py
(every encoder and decoder path on those inputs).

ROWS is typed in from the reference's C# -- the LzProperties of each class and the places where its writer changes token form -- and is NOT read
from the library (alz_encode_geometry) or from the oracle (props_for): a disagreement between the three is a finding.  Paths are relative to the
reference's src/; `oracle:` names the function of oracle/alz_oracle.c that restates the writer.

A step `s` in len_steps / dist_steps / lit_steps means "the form changes between s and s + 1": both sides are planted.  tests/test_geometry_edges_cpu.py
holds the steps against the writers' sizes: a token's or a literal run's size changes at the listed places and nowhere else (Row.silent: the listed form changes that
leave the size alone).

planted(row) -> (data, plants): ONE stream per row.  It starts with a filler in which no group of `gram` bytes occurs twice (gram = min(min_len, 4):
the finder hashes four bytes, so four distinct bytes are as good as five), followed by plants -- copies of data[p - d : p - d + n] written byte by
byte, so that n > d works -- each behind a run of fresh bytes and in front of a separator whose first byte differs from the byte that would lengthen
the match.  "Fresh" means: every group of `gram` bytes that contains the byte is new to the whole stream, so a plant's only earlier occurrence is
its source.  check_stream() verifies that with a set of n-grams instead of assuming it."""
import functools
import random

import numpy as np

import chain_finder_ref as CF
from auroralib.compression_amd import _abi as A

INF = 0x7FFFFFFF                                     # int.MaxValue: "unbounded"


class Row:
    def __init__(self, name, fmt, props, cite, len_steps=(), dist_steps=(), lit_steps=(), flag_bits=False, kw=None, end_guard=8, silent=()):
        self.name, self.fmt, self.cite = name, fmt, cite
        self.props = props                           # [(max_dist, max_len, min_len, min_dist)]: the finder's property sets, in the class's order
        self.len_steps, self.dist_steps, self.lit_steps = tuple(len_steps), tuple(dist_steps), tuple(lit_steps)
        self.silent = frozenset(silent)             # the listed steps at which the form changes and the token's SIZE does not (bits move inside the opcode)
        self.flag_bits = flag_bits                   # flag-bit format: 8 phases; otherwise the 64 lanes of the window walk
        self.kw = dict(kw or {})                     # encode settings, as O.encode_stream / Context.encode_batch take them
        self.end_guard = end_guard                   # fresh bytes behind the last plant (LZ4 stops searching 5 bytes before the end, LZ4.cs:208)
        self.min_len = min(p[2] for p in props)
        self.max_len = max(p[1] for p in props)
        self.max_dist = max(p[0] for p in props)
        self.min_dist = min(p[3] for p in props)
        self.gram = min(self.min_len, 4)
        self.decodable = True                        # the reference's own reader reads back what its writer wrote ...
        self.decodable_from = 0                      # ... from this quality on

    def finder_props(self):
        return [CF.LzProperties(md, ml, mn, 0, nd) for md, ml, mn, nd in self.props]

    def finder_kw(self):
        return dict(max_window_bits=self.kw.get("max_window_bits", 0), strategy=self.kw.get("strategy", 0))

    def admits(self, d, n):
        """The length ScoreMatch (LzChainMatchFinder.cs:301-321) gives a candidate of n equal bytes at distance d: the FIRST set that admits it
        clamps it; 0 where none does."""
        if self.kw.get("strategy", 0) & 1 and n > d:
            n = d
        for md, ml, mn, nd in self.props:
            if nd <= d <= md and n >= mn:
                return min(n, ml)
        return 0

    def __repr__(self):
        return self.name


def _lzss(bits, **kw):
    b, l, t = bits
    # LzProperties(byte distanceBits, byte lengthBits, byte threshold)  LzProperties.cs:57-66: window 1 << b, lengths t + 1 .. (1 << l) + t
    row = Row("lzss_%d_%d_%d%s" % (b, l, t, "_compat" if kw.get("strategy") else ""), A.FMT_LZSS, [(1 << b, (1 << l) + t, t + 1, 1)],
              "LzProperties.cs:57-66, LZSS.cs:33, writer LZSS.cs:132-160 (oracle: enc_lzss)", flag_bits=True,
              kw=dict(lz=A.LzProperties.from_bits(b, l, t), **kw))
    # the writer casts the token to a ushort (LZSS.cs:156): with more than 16 bits of distance and length the high distance bits are lost and the body does not
    # decode -- in the reference either.  Such geometries are compared byte for byte and not decoded back.
    row.decodable = b + l <= 16
    return row


_FLAG18 = dict(flag_bits=True)
ROWS = [
    _lzss((8, 4, 2)), _lzss((12, 4, 2)), _lzss((14, 4, 2)), _lzss((15, 6, 2)), _lzss((16, 8, 2)),
    _lzss((12, 4, 2), strategy=1),                                                                    # CompatibilityMode: no self-overlap, LzChainMatchFinder.cs:303-304
    Row("lz10", A.FMT_LZ10, [(0x1000, 18, 3, 1)], "LZ10.cs:25, writer :113-137 (oracle: enc_lz10)", **_FLAG18),
    Row("lz10_vram", A.FMT_LZ10, [(0x1000, 18, 3, 2)], "LZ10.cs:30 (_lzVram)", kw=dict(min_distance=2), **_FLAG18),
    Row("lz11", A.FMT_LZ11, [(0x1000, 0x4000, 3, 1)], "LZ11.cs:25, writer :135-171 (oracle: enc_lz11)", len_steps=(16, 272), **_FLAG18),
    Row("lz11_vram", A.FMT_LZ11, [(0x1000, 0x4000, 3, 2)], "LZ11.cs:26 (_lzVram)", len_steps=(16, 272), kw=dict(min_distance=2), **_FLAG18),
    Row("lz40", A.FMT_LZ40, [(0x1000, 0x4000, 3, 1)], "LZ40.cs:25, writer :134-176 (oracle: enc_lz40)", len_steps=(15, 271), **_FLAG18),
    Row("yaz0", A.FMT_YAZ0, [(0x1000, 0xFF + 0x12, 3, 1)], "Yay0.cs:27, writer Yay0.cs:152-184 through Yaz0.cs:94-98 (oracle: enc_yay0_core)", len_steps=(17,), **_FLAG18),
    Row("yay0", A.FMT_YAY0, [(0x1000, 0xFF + 0x12, 3, 1)], "Yay0.cs:27, writer :152-184 (oracle: enc_yay0_core)", len_steps=(17,), **_FLAG18),
    Row("lzhudson", A.FMT_LZHUDSON, [(0x1000, 0xFF + 18, 3, 1)], "LZHudson.cs:24, writer Yay0.cs:152-184 through LZHudson.cs:55-59", len_steps=(17,), **_FLAG18),
    Row("mio0", A.FMT_MIO0, [(0x1000, 18, 3, 1)], "MIO0.cs:28, writer :159-184 (oracle: enc_mio0_core)", **_FLAG18),
    Row("smsr00", A.FMT_SMSR00, [(0x1000, 18, 3, 1)], "SMSR00.cs:29, writer MIO0.cs:159-184 through SMSR00.cs:133-137", **_FLAG18),
    Row("clz0", A.FMT_CLZ0, [(0x1000, 18, 3, 1)], "CLZ0.cs:26, writer :99-130 (oracle: enc_clz0)", **_FLAG18),
    Row("blz", A.FMT_BLZ, [(0x1000, 18, 3, 3)], "BLZ.cs:24 (minDistance 3), writer :137-216 (oracle: enc_blz)", **_FLAG18),
    # PRS: short form for lengths 2..5 at distances <= 0x100, long form with a length byte from 10 on; a 2-byte match beyond 0x100 is dropped (PRS.cs:124-125)
    Row("prs_be", A.FMT_PRS_BE, [(0x1FFF, 0x100, 2, 1)], "PRS.cs:21, writer :104-159 (oracle: enc_prs)", len_steps=(5, 9), dist_steps=(0x100,), **_FLAG18),
    Row("prs_le", A.FMT_PRS_LE, [(0x1FFF, 0x100, 2, 1)], "PRS.cs:21, writer :104-159 (oracle: enc_prs)", len_steps=(5, 9), dist_steps=(0x100,), **_FLAG18),
    # LZ4: the token holds length - 4 up to 14 and literal counts up to 14; one extension byte holds 254 more (LZ4.cs:254-268)
    Row("lz4_block", A.FMT_LZ4_BLOCK, [(0xFFFF, INF, 4, 1)], "LZ4.cs:29, writer :202-238, WriteExtension :254-268 (oracle: enc_lz4)",
        len_steps=(18, 273), lit_steps=(14, 269), end_guard=64),
    # LZO: M2 (length <= 8, distance <= 2048; its two opcodes split at length 4), M3 (distance <= 16384; length in the opcode up to 33), M4 (up to 9);
    # literal runs: 1..3 ride in the token in front, up to 18 in one byte, then an extension chain (+255)
    Row("lzo", A.FMT_LZO, [(0xBFFF, INF, 3, 1)], "LZO.cs:24, writer :141-250, WriteExtendedInt :263-271 (oracle: enc_lzo)",
        len_steps=(4, 8, 9, 33), dist_steps=(2048, 16384), lit_steps=(3, 18, 273), end_guard=64, silent=(4,)),
    # Snappy: copy-1 for lengths 4..11 at distances < 2048, else copy-2; literal runs up to 60 in the tag, up to 256 with one length byte
    Row("snappy_raw", A.FMT_SNAPPY_RAW, [(0x8000, 63 + 1, 4, 1)], "Snappy.cs:28, writer :124-203 (oracle: enc_snappy)",
        len_steps=(11,), dist_steps=(2047,), lit_steps=(60, 256)),
    # FastLZ level 1: length - 3 up to 6 in the opcode, a length byte from 9 on; literal runs of at most 32
    Row("fastlz", A.FMT_FASTLZ, [(0x2000, 0xFF + 3 + 6, 3, 1)], "FastLZ.cs:22, writer :162-245 (oracle: enc_fastlz)", len_steps=(8,), lit_steps=(32,)),
    # FastLZ level 2 (source >= 64 KiB, Quality > 4, MaxWindowBits > 13  FastLZ.cs:169-175): two sets; 255-chains of length bytes; distances from 0x2000 on
    # take two more bytes (distance - 1 >= 0x1FFF  :229-235)
    Row("fastlz_level2", A.FMT_FASTLZ, [(0x1FFF, INF, 3, 1), (0x11FFF, INF, 5, 1)], "FastLZ.cs:25-26, writer :162-245 (oracle: enc_fastlz)",
        len_steps=(8, 263), dist_steps=(0x1FFF,), lit_steps=(32,), kw=dict(max_window_bits=17)),
    # CNX2: a single literal has a form of its own, runs hold up to 255
    Row("cnx2", A.FMT_CNX2, [(0x800, 0x1F + 4, 4, 1)], "CNX2.cs:26, writer :140-172 (oracle: enc_cnx2)", lit_steps=(1, 255), flag_bits=True),
    Row("cns", A.FMT_CNS, [(0x100, 130, 3, 1)], "CNS.cs:26, writer :111-141 (oracle: enc_cns)", lit_steps=(127,)),
    Row("lz02", A.FMT_LZ02, [(0xFFF, 272, 3, 1)], "LZ02.cs:26, writer :117-151 (oracle: enc_lz02)", len_steps=(16,), flag_bits=True),
    # LZShrek: lengths up to 7 in the token; distances up to 30 in the token, up to 286 with one byte; literal counts up to 29 / 285 likewise
    Row("lzshrek", A.FMT_LZSHREK, [(0x1000, 262, 3, 1)], "LZShrek.cs:23, writer :121-174 (oracle: enc_lzshrek)",
        len_steps=(7,), dist_steps=(30, 286), lit_steps=(29, 285)),
    # HIG: short form (distance <= 0x7FF, length <= 9), middle form (distance <= 0x3FFF, length <= 35), long form with the length in the opcode up to 18,
    # in a byte up to 273, then as a ushort; literal blocks of 1..2 ride in the token, up to 257 have a count byte
    Row("hig", A.FMT_HIG, [(0x7FFF, 0xFFFF, 4, 1)], "HIG.cs:28, writer :214-323 (oracle: enc_hig)",
        len_steps=(9, 18, 35, 273), dist_steps=(0x7FF, 0x3FFF), lit_steps=(2, 257)),
    # WFLZ: a block carries at most 255 literals; min length 4 + 1
    Row("wflz", A.FMT_WFLZ, [(0xFFFF, 0xFF, 5, 1)], "WFLZ.cs:22, writer :161-196 (oracle: enc_wflz)", lit_steps=(255,)),
    Row("wflz_be", A.FMT_WFLZ_BE, [(0xFFFF, 0xFF, 5, 1)], "WFLZ.cs:22, writer :161-196 (oracle: enc_wflz)", lit_steps=(255,)),
    # RefPack: long / medium / short form; the long form's distance and length have high bits in the opcode (0x10000; 256 steps of length - 5);
    # literal runs up to 3 ride in the token, stored runs hold at most 0x70 (and three more ride: a second stored run from 0x74 on)
    Row("refpack", A.FMT_REFPACK, [(0x20000, 1028, 5, 1), (0x4000, 67, 4, 1), (0x400, 10, 3, 1)], "RefPack.cs:35-37, writer :241-303 (oracle: enc_refpack)",
        len_steps=(10, 67, 260, 516, 772), dist_steps=(0x10000,), lit_steps=(3, 0x70, 0x73), silent=(260, 516, 772, 0x10000, 0x70)),
]
BY_NAME = {r.name: r for r in ROWS}
BY_NAME["fastlz_level2"].decodable_from = 5         # (below Quality 5 the same settings give level 1 with a finder window the format cannot store: FastLZ.cs:169-175)
assert sorted({r.fmt for r in ROWS}) == list(range(A.FMT_COUNT))               # every format of the main codec has a row


# ------------------------------------------------------------------------------------------------ the builder
class _Builder:
    def __init__(self, gram, seed):
        self.b, self.g, self.seen, self.rng = bytearray(), gram, set(), random.Random(seed)
        self.copied, self.run_bytes, self.fresh_mask = [], set(), bytearray()

    def filler(self, n):
        """n bytes whose groups of `gram` bytes are all different: random bytes with every repeat redrawn (for two-byte groups -- PRS -- that is a walk that
        never takes an edge of the 256 x 256 graph twice)."""
        if self.g < 3:
            return self.fresh(n)
        rs = np.random.default_rng(self.rng.getrandbits(32))
        a = rs.integers(0, 256, n, dtype=np.uint8)
        while True:
            v = np.zeros(n - self.g + 1, dtype=np.uint64)
            for k in range(self.g):
                v |= a[k:n - self.g + 1 + k].astype(np.uint64) << np.uint64(8 * k)
            _, first, counts = np.unique(v, return_index=True, return_counts=True)
            if counts.max() == 1:
                break
            dup = np.setdiff1d(np.arange(len(v)), first)
            a[dup] = rs.integers(0, 256, len(dup), dtype=np.uint8)
        assert not self.b
        self.b += a.tobytes()
        self.fresh_mask += b"\x01" * n
        g = self.g
        self.seen.update(bytes(self.b[i:i + g]) for i in range(n - g + 1))

    def fresh(self, k, avoid=None, log=None):
        b, g = self.b, self.g
        for i in range(k):
            for _try in range(100000):
                c = self.rng.randrange(256)
                if i == 0 and c == avoid:
                    continue
                key = bytes(b[len(b) - g + 1:]) + bytes([c]) if len(b) >= g - 1 else None
                if key is None or key not in self.seen:
                    break
            else:
                raise AssertionError("no fresh byte left")
            if key is not None:
                self.seen.add(key)
                if log is not None:
                    log.append(key)
            b.append(c)
            self.fresh_mask.append(1)

    def plant(self, d, n, gap, avoid=None, run=False):
        """`gap` fresh bytes (more where the source would otherwise lie inside an earlier plant), then n bytes copied from distance d.  Returns the plant's position."""
        b, g = self.b, self.g
        while True:
            lo = len(b) + gap - d
            assert lo >= 0, (len(b), gap, d)
            hit = [e for s, e in self.copied if s < lo + n + 1 and lo < e]
            if not hit:
                break
            gap = max(hit) + d - len(b)
        for _try in range(1000):
            mark, log = len(b), []
            self.fresh(gap, avoid=avoid, log=log)
            if d == 1 and b[-1] in self.run_bytes:         # (runs of one byte value each: two runs of the same value would be each other's candidates)
                ok = False
            elif len(b) > d and b[-1] == b[-1 - d]:              # (the byte in front would lengthen the match backwards)
                ok = False
            else:
                follow = bytearray()                               # the first bytes of the copy: the groups that straddle its start must be new as well
                for i in range(min(n, g - 1)):
                    at = len(b) + i - d
                    follow.append(b[at] if at < len(b) else follow[at - len(b)])
                span = [bytes(b[len(b) - (g - j):]) + bytes(follow[:j]) for j in range(1, len(follow) + 1) if len(b) >= g - j]
                ok = not any(s in self.seen for s in span)
            if ok:
                break
            for key in log:
                self.seen.discard(key)
            del b[mark:]
            del self.fresh_mask[mark:]
        else:
            raise AssertionError("no separator fits in front of the plant")
        if d == 1:
            self.run_bytes.add(b[-1])
        p = len(b)
        for _ in range(n):
            b.append(b[len(b) - d])
            self.fresh_mask.append(0)
        for i in range(max(0, p - g + 1), len(b) - g + 1):
            self.seen.add(bytes(b[i:i + g]))
        self.copied.append((p, p + n))
        self.avoid = b[p - d + n]                                  # the byte that would lengthen the match
        return p


def _window_lengths(row, md, ml, mn):
    out = {mn, mn + 1, 4, max(9, mn + 4), 10, 11}          # (4: the shortest repeat a hash of four bytes finds)
    for s in row.len_steps:
        out |= {s, s + 1}
    if ml <= 0x10000:
        out.add(ml)
        if ml <= 0x4000:
            out.add(ml - 1)
    return sorted(n for n in out if mn <= n <= ml)


def _clamp_cases(row):
    """(period, k): available match length max_len + k, for k = -1 .. min_len + 2 (every remainder a clamped match can leave that the finder may or may not take) and
    max_len + 1 (two clamped matches and one byte).  Periods 1, 3 and 64 -- for the formats whose max_len is 16 KiB (LZ11, LZ40) period 3 alone and for HIG (64 KiB)
    period 1 alone, every k: the other two periods would add 0.3 MB and 1.3 MB of run to streams every GPU path encodes at three qualities."""
    ml, mn = row.max_len, row.min_len
    if ml >= INF:
        return []
    ks = list(range(-1, mn + 3)) + [ml + 1]                        # (max_len + (max_len + 1) = 2 * max_len + 1)
    periods = (1,) if ml > 0x4000 else (3,) if ml > 2048 else (1, 3, 64)
    return [(P, k) for P in periods for k in ks]


@functools.lru_cache(maxsize=None)
def _planted(name, seed, short, lead):
    row = BY_NAME[name]
    bl = _Builder(row.gram, seed * 1000003 + sum(name.encode()))
    plants = []
    if lead:
        bl.fresh(lead)
    base = len(bl.b)
    size = max(row.max_dist + 64, 24 << 10)                        # (24 KiB: what the whole-GPU paths take)
    if lead:
        bl.fresh(size)                                             # (drawn like every other fresh byte: the numpy filler wants an empty stream)
    else:
        bl.filler(size)
    filler_end = len(bl.b)
    bl.avoid = None

    def put(kind, d, n, gap, **kw):
        p = bl.plant(d, n, gap, avoid=bl.avoid, **kw)
        plants.append(dict(kind=kind, p=p, d=d, n=n))
        return p

    # ---- window: every tier's last distances with every length class; the other distances with a few lengths
    todo = []
    small = sorted({row.min_len, row.min_len + 1, row.min_len + 2, 5, 9, 10, 11})
    for md, ml, mn, nd in row.props:
        for n in ([mn, max(9, mn + 4)] if short else _window_lengths(row, md, ml, mn)):
            todo.append((md, n))
        for d in (md - 1, md + 1):
            todo += [(d, n) for n in ((9,) if short else small)]
    for s in row.dist_steps:
        todo += [(d, n) for d in (s, s + 1) for n in ((9,) if short else small)]
    for d, n in sorted(set(todo), key=lambda t: (-t[0], t[1])):
        put("window", d, n, 6)
    if not short:
        # ---- near: distances 1, 2, 3 and around min_dist, with the self-overlapping lengths
        for d in sorted({1, 2, 3, row.min_dist - 1, row.min_dist, row.min_dist + 1} - {0}):
            for n in sorted({d - 1, d, d + 1, 2 * d + 1, row.min_len, row.min_len + d, 12} - {0}):
                put("near", d, n, max(d, 4) + 2)
        # ---- clamp: periodic runs whose available match length is max_len + k
        for P, k in _clamp_cases(row):
            p = put("clamp", P, row.max_len + k, max(P, 4), run=True)
            plants[-1].update(period=P, k=k)
        # ---- literal runs: s and s + 1 fresh bytes between two short plants whose sources lie in a fresh block of their own
        for s in row.lit_steps:
            for run in (s, s + 1):
                bl.fresh(44, avoid=bl.avoid)
                f0 = len(bl.b) - 40
                put("lit", len(bl.b) + 4 - f0, 9, 4)
                put("lit", len(bl.b) + run - (f0 + 12), 9, run)
                plants[-1]["run"] = run
    bl.fresh(max(row.end_guard, 8), avoid=bl.avoid)
    data = bytes(bl.b)
    return data, plants, (base, filler_end), bytes(bl.fresh_mask)


def planted(row, seed=1):
    """(data, plants) of the row's full corpus."""
    data, plants, _, _ = _planted(row.name, seed, False, 0)
    return data, plants


def phases(row, seed=1):
    """The short corpus (window plants only) behind 0..7 extra leading literals for the flag-bit formats, 0..63 for the formats of the 64-position window walk:
    ONE stream built behind the longest lead, and its suffixes -- a suffix keeps every property of the stream."""
    k = 8 if row.flag_bits else 64
    data, plants, _, _ = _planted(row.name, seed, True, k - 1)
    return [data[k - 1 - i:] for i in range(k)]


def check_stream(row, seed=1, short=False, lead=0):
    """The conditions the builder promises, checked independently of it with a table of n-grams: (1) a group of `gram` bytes that contains a fresh byte occurs once
    in the whole stream; (2) so the filler has no repeated group; (3) every plant is a copy of its source and the byte behind it differs from the one behind
    the source."""
    data, plants, (f0, f1), fresh = _planted(row.name, seed, short, lead)
    g = row.gram
    where = {}
    for i in range(len(data) - g + 1):
        where.setdefault(data[i:i + g], []).append(i)
    for key, at in where.items():                                  # (a plant repeats its source's groups: all but one occurrence lie wholly inside copies)
        if len(at) > 1:
            assert sum(1 for i in at if any(fresh[i:i + g])) <= 1, (row.name, "a group with a fresh byte occurs twice outside the plants", at[:4])
    assert f1 - f0 >= row.max_dist + 64 and all(fresh[f0:f1])
    for pl in plants:
        p, d, n = pl["p"], pl["d"], pl["n"]
        assert all(data[p + i] == data[p + i - d] for i in range(n)), pl
        assert data[p + n] != data[p + n - d] and (p - 1 - d < 0 or data[p - 1] != data[p - 1 - d]), pl
        assert fresh[p - 1] and fresh[p + n], pl
    return data, plants
