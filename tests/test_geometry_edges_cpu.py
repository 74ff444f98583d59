"""No GPU: the inputs of tests/geometry_cases.py prove themselves.  For every row of its table, from the reference side alone (the oracle and the finder
restatement, tests/chain_finder_ref.py, with the row's own properties):

  * the builder's promises hold (no repeated group in the filler, every plant a copy of its source that nothing lengthens: geometry_cases.check_stream);
  * the oracle's body decodes back to the input, and its SIZE is the size the row's writer gives the finder's token list (body_size below restates, per
    writer, how many bytes a literal run and a match of a given length and distance take -- the token-form steps of the table).  The oracle returns bytes,
    not tokens, so this is how the finder is pinned to it for every format: a literal or a match more or less, or a step off by one, changes the size;
  * at quality 8 the token list has a match at exactly max_dist -- and at the last distance of every tier and form --, none beyond max_dist, a plant one past
    a tier only with the length the outer tier demands, a match of exactly max_len where that is finite, a token on each side of every length step, a literal
    run on each side of every literal-run step;
  * a match of exactly min_len: at quality 8 where min_len >= 4.  THE ONE CLASS THAT QUALITY 8 CANNOT REACH for min_len < 4: the finder looks candidates up
    by a hash of FOUR bytes (LzChainMatchFinder.cs:288-299), and a repeat of exactly three bytes differs from its source in the fourth.  Such matches come from
    the min-length table, which exists from quality 10 on (:100-104, :226-243): they are asserted at quality 12, on the near plants;
  * what the finder does behind a clamped match, for every remainder, is the list committed in tests/golden/geometry_clamp.json (make_geometry_clamp.py).

The same plants are encoded through the oracle with and without them (fresh bytes in their place): "taken" also means that the body gets smaller."""
import functools
import json
import os
import random

import pytest

import chain_finder_ref as CF
import geometry_cases as G
from auroralib.compression_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_IDS = [r.name for r in G.ROWS]


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib as O
    return O


@functools.lru_cache(maxsize=None)
def finder_tokens(name, quality):
    row = G.BY_NAME[name]
    data, _ = G.planted(row)
    if row.fmt == A.FMT_LZ4_BLOCK:                       # the finder sees all but the last five bytes  LZ4.cs:208
        data = data[:-5]
    return CF.matches(row.finder_props(), data, quality, **row.finder_kw())


# ------------------------------------------------------------------------------------------------ the writers, as sizes
def _ext255(v, first):
    """extension bytes of a count whose opcode holds `first` - 1: one byte per 255 (LZ4.cs:254-268)"""
    return 0 if v < first else 1 + (v - first) // 255


def _lzo_ext(v):                                        # LZO.cs:263-271: zero bytes while v > 255, then v
    n = 1
    while v > 255:
        n += 1; v -= 255
    return n


def body_size(row, data, toks):
    """The size of the body the row's writer makes of `toks` ((offset, distance, length)..., (len(data), 0, 0))."""
    f = row.fmt
    n_data = len(data)
    runs, sp = [], 0                                     # the literal run in front of every entry
    for o, d, n in toks:
        runs.append(o - sp); sp = o + n
    lits, ms = sum(runs), [(d, n) for _, d, n in toks if n]
    ntok = lits + len(ms)
    if f in (A.FMT_LZSS, A.FMT_LZ10, A.FMT_BLZ, A.FMT_CLZ0):
        return -(-ntok // 8) + lits + 2 * len(ms)
    if f == A.FMT_LZ11:                                  # LZ11.cs:150-164
        return -(-ntok // 8) + lits + sum(2 if n <= 16 else 3 if n <= 272 else 4 for _, n in ms)
    if f == A.FMT_LZ40:                                  # LZ40.cs:150-168
        return -(-ntok // 8) + lits + sum(2 if n < 16 else 3 if n < 272 else 4 for _, n in ms)
    if f in (A.FMT_YAZ0, A.FMT_YAY0):                    # Yay0.cs:165-177
        return -(-ntok // 8) + lits + sum(2 if n < 18 else 3 for _, n in ms)
    if f == A.FMT_LZHUDSON:                              # 32 flag bits at a time  LZHudson.cs:55-59
        return 4 * -(-ntok // 32) + lits + sum(2 if n < 18 else 3 for _, n in ms)
    if f == A.FMT_MIO0:
        return -(-ntok // 8) + lits + 2 * len(ms)
    if f == A.FMT_SMSR00:                                # 16 flag bits at a time  SMSR00.cs:133-137
        return 2 * -(-ntok // 16) + lits + 2 * len(ms)
    if f == A.FMT_LZ02:                                  # LZ02.cs:133-149: the terminator is a token of its own
        return -(-(ntok + 1) // 8) + lits + sum(2 if n <= 16 else 3 for _, n in ms) + 2
    if f == A.FMT_CNS:                                   # CNS.cs:121-137
        return sum(r + -(-r // 127) for r in runs) + 2 * len(ms)
    if f == A.FMT_CNX2:                                  # CNX2.cs:150-168: two flag bits per element
        el = by = 0
        for r in runs:
            while r:
                c = min(r, 255)
                el += 1; by += 1 if c == 1 else 1 + c; r -= c
        return -(-2 * (el + len(ms)) // 8) + by + 2 * len(ms)
    if f in (A.FMT_PRS_BE, A.FMT_PRS_LE):                # PRS.cs:117-157
        bits = by = 0
        for (o, d, n), r in zip(toks, runs):
            bits += r; by += r
            if n == 0:
                break
            if n == 2 and d > 0x100:                     # dropped: its two bytes are literals of the next round  :124-125
                bits += 2; by += 2
            elif d <= 0x100 and n <= 5:
                bits += 4; by += 1
            else:
                bits += 2; by += 3 if n > 9 else 2
        return -(-(bits + 2) // 8) + by + 2
    if f == A.FMT_LZ4_BLOCK:                             # LZ4.cs:212-236
        size = 0
        for (o, d, n), r in zip(toks, runs):
            if n == 0:
                r += 5                                   # (the five bytes the finder did not see)
                return size + 1 + _ext255(r, 15) + r
            size += 1 + _ext255(r, 15) + r + 2 + _ext255(n - 4, 15)
    if f == A.FMT_SNAPPY_RAW:                            # Snappy.cs:131-200
        size, v = 1, n_data
        while v >= 0x80:
            size += 1; v >>= 7
        for r in runs:
            if r:
                size += r + (1 if r <= 60 else 2 if r <= 256 else 3)
        return size + sum(2 if d < 2048 and 4 <= n <= 11 else 3 for d, n in ms)
    if f == A.FMT_FASTLZ:                                # FastLZ.cs:181-235
        l2 = len(row.props) == 2
        size = sum(r + -(-r // 32) for r in runs)
        for d, n in ms:
            size += 2 + (0 if n - 3 < 6 else 1 + ((n - 9) // 255 if l2 else 0)) + (2 if l2 and d - 1 >= 0x1FFF else 0)
        return size
    if f == A.FMT_REFPACK:                               # RefPack.cs:257-301
        size = 0
        for (o, d, n), r in zip(toks, runs):
            while r > 3:
                c = (min(r, 0x70) // 4 - 1) * 4 + 4
                size += 1 + c; r -= c
            if n == 0:
                return size + 1 + r
            size += r + (2 if n <= 10 and d <= 0x400 else 3 if 4 <= n <= 67 and d <= 0x4000 else 4)
    if f in (A.FMT_WFLZ, A.FMT_WFLZ_BE):                 # WFLZ.cs:169-194: a block per match with up to 255 of the literals behind it; further literals in blocks of their own
        size, sp, i = 0, 0, 0
        mo = mn = 0
        plain = toks[0][0]
        while True:
            bp = min(plain, 255)
            size += 4 + bp; plain -= bp; sp += mn + bp
            if plain == 0:
                if sp == n_data:
                    return size + 4
                mo, _, mn = toks[i]
                i += 1
                plain = toks[i][0] - (mo + mn)
            else:
                mo = mn = 0
    if f == A.FMT_LZSHREK:                               # LZShrek.cs:129-173
        size, i, sp = 0, 0, 0
        while sp != n_data:
            plain = toks[i][0] - sp
            sp += plain
            comp = 0
            while toks[i][2] and comp < 8 and toks[i][0] == sp:
                o, d, n = toks[i]
                size += 1 + (1 if n > 7 else 0) + (0 if d <= 30 else 1 if d <= 286 else 2)
                sp += n; i += 1
                if toks[i][2] == 0 or comp >= 7 or toks[i][0] != sp:
                    break
                comp += 1
            size += 1 + plain + (0 if plain <= 29 else 1 if plain <= 285 else 2)
        return size + 4
    if f == A.FMT_HIG:                                   # HIG.cs:214-323
        raw = lambda p: 1 if p <= 257 else 3             # noqa: E731
        it = iter(toks)
        o, d, n = next(it)
        plain = o
        if plain < 2:
            n -= plain + 1; o = 2; plain = 2
            if n < 4:
                o, d, n = next(it); plain = o
        size = raw(plain) + plain
        while n:
            no, nd, nn = next(it)
            plain = no - (o + n)
            if d <= 0x7FF and n <= 9:
                size += 1
            else:
                if d <= 0x3FFF and n <= 35:
                    size += 1
                else:
                    size += 1 + (0 if n <= 18 else 1 if n <= 273 else 3)
                size += 1
            size += 1
            if plain:
                size += plain + (raw(plain) if plain > 2 else 0)
            o, d, n = no, nd, nn
        return size
    if f == A.FMT_LZO:                                   # LZO.cs:141-250
        it = iter(toks + [toks[-1]] * 2)
        size, sp = 0, 0
        (o, d, n), (no, nd, nn) = next(it), next(it)
        while sp != n_data:
            plain = o - sp
            if plain:
                if plain < 4:
                    o += 4 - plain; n -= 4 - plain; plain = 4
                size += (1 + _lzo_ext(plain - 18) if plain > 18 else 1) + plain
                sp += plain
            if n >= 3:
                sp += n
                plain = no - sp
                if plain > 3:
                    plain = 0
                assert plain >= 0
                if n <= 8 and d <= 2048:
                    size += 2
                elif d <= 16384:
                    size += (1 + _lzo_ext(n - 33) if n > 33 else 1) + 2
                else:
                    size += (1 + _lzo_ext(n - 9) if n > 9 else 1) + 2
                size += plain; sp += plain
            (o, d, n), (no, nd, nn) = (no, nd, nn), next(it)
        return size + 3
    raise AssertionError(row.name)


def _repeated_cost(row, d, n, run=8, reps=8, first=None):
    """body_size of `reps` matches (d, n), each behind `run` literals (the first behind `first`): eight times a token's own size shows through the rounding of flag
    bits to bytes.  Without Snappy's length prefix, which grows with the input."""
    toks, pos = [], (run if first is None else first) - run
    for _ in range(reps):
        pos += run
        toks.append((pos, d, n)); pos += n
    toks.append((pos + 8, 0, 0))
    total = pos + 8 + (5 if row.fmt == A.FMT_LZ4_BLOCK else 0)
    prefix = len(bin(total)) - 2 if row.fmt == A.FMT_SNAPPY_RAW else 0
    return body_size(row, bytes(total), toks) - -(-prefix // 7)


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_listed_steps_are_where_the_writers_size_changes(name):
    """The token-form steps of the table against body_size (which the oracle's bodies pin, above): the size of a match changes with its length exactly at the row's
    len_steps, with its distance exactly at its dist_steps (or at a tier's last distance), and a literal run's overhead changes exactly at its lit_steps -- apart from
    Row.silent, the listed form changes that move bits inside an opcode.  Distances are sampled: every one up to 5 000, and around every power of two and every listed one."""
    row = G.BY_NAME[name]
    tiers = {p[0] for p in row.props}
    dists = set(range(max(row.min_dist, 1), min(row.max_dist, 5000) + 1))
    for c in [1 << k for k in range(2, 18)] + list(row.dist_steps) + sorted(tiers):
        dists |= {d for d in range(c - 3, c + 4) if row.min_dist <= d <= row.max_dist}
    dists = sorted(dists)
    lens = sorted({n for n in range(row.min_len, min(row.max_len, 1100) + 1)})
    # ---- lengths: at a few distances of every form
    found = set()
    for d in sorted({row.min_dist, *(x for s in row.dist_steps for x in (s, s + 1)), *tiers, *(t + 1 for t in tiers if t < row.max_dist)}):
        ok = [n for n in lens if row.admits(d, n) == n and not (row.fmt in (A.FMT_PRS_BE, A.FMT_PRS_LE) and n == 2)]
        cost = [(n, _repeated_cost(row, d, n)) for n in ok]
        found |= {a for (a, fa), (b, fb) in zip(cost, cost[1:]) if b == a + 1 and fb != fa}
    listed = {s for s in row.len_steps if s < 1100}
    if listed:                                           # (beyond the last listed step a chain of extension bytes repeats it every 255)
        found = {n for n in found if n <= max(listed) + 1}
    assert found <= listed and listed - row.silent <= found, (name, "length steps", sorted(found), sorted(listed))
    # ---- distances: at a few lengths of every form
    found = set()
    for n in sorted({x for s in row.len_steps if s < 1100 for x in (s, s + 1)} | {row.min_len, max(p[2] for p in row.props), 20}):
        ok = [d for d in dists if row.admits(d, n) == n and not (row.fmt in (A.FMT_PRS_BE, A.FMT_PRS_LE) and n == 2)]
        cost = [(d, _repeated_cost(row, d, n)) for d in ok]
        found |= {a for (a, fa), (b, fb) in zip(cost, cost[1:]) if b == a + 1 and fb != fa}
    listed = set(row.dist_steps)
    assert found <= listed | tiers and listed - row.silent <= found, (name, "distance steps", sorted(found), sorted(listed))
    # ---- literal runs (the formats that count them; under flag bits every literal costs the same nine bits)
    if not row.flag_bits:
        d = min(20, row.max_dist)
        cost = [(r, _repeated_cost(row, d, 9, run=r, reps=2, first=40)) for r in range(4, 700)]
        found = {a for (a, fa), (b, fb) in zip(cost, cost[1:]) if fb - fa != 1}
        small = [(r, _repeated_cost(row, d, 9, run=r, reps=2, first=40)) for r in range(1, 6)]
        found |= {a for (a, fa), (b, fb) in zip(small, small[1:]) if fb - fa != 1}
        top = max(row.lit_steps) + 1 if row.lit_steps else 700
        listed = set(row.lit_steps)
        assert {r for r in found if r <= top} <= listed and listed - row.silent <= found, (name, "literal-run steps", sorted(found)[:8], sorted(listed))


def _oracle_body(O, row, data, quality):
    return O.encode_stream(row.fmt, data, quality=quality, **row.kw)


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_builder_keeps_its_promises(name):
    row = G.BY_NAME[name]
    G.check_stream(row)
    G.check_stream(row, short=True, lead=(8 if row.flag_bits else 64) - 1)
    data, _ = G.planted(row)
    assert len(data) >= 24 << 10 and all(len(s) > row.max_dist for s in G.phases(row))


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_oracle_round_trips_and_its_size_is_the_finders_tokens_through_the_rows_writer(name, oracle):
    row = G.BY_NAME[name]
    data, _ = G.planted(row)
    for q in (8, 12):
        body, aux = _oracle_body(oracle, row, data, q)
        back, r = oracle.decode_stream(row.fmt, body, decom_len=len(data), cap=len(data), aux0=aux.aux0, aux1=aux.aux1, lz=row.kw.get("lz"))
        assert (r.status == A.ST_OK and back == data) == row.decodable, (name, q, r.status, r.dst_len)
        toks = finder_tokens(name, q)
        assert body_size(row, data, toks) == len(body), (name, q, sum(1 for t in toks if t[2]))


def _expected(row, pl, quality):
    """the token at a plant: (distance, length), or None where the finder must pass it by"""
    n = row.admits(pl["d"], pl["n"])
    if n and pl["n"] < 4 and quality < 10:               # (the hash is of four bytes: see the module's text)
        return "either"
    return (pl["d"], n) if n else None


@pytest.mark.parametrize("name", ROW_IDS)
def test_window_plants_are_taken_up_to_every_limit_and_not_beyond(name, oracle):
    row = G.BY_NAME[name]
    data, plants = G.planted(row)
    by_off = {o: (d, n) for o, d, n in finder_tokens(name, 8) if n}
    covered = sorted((o, o + n) for o, (d, n) in by_off.items())
    seen = set()
    for pl in plants:
        if pl["kind"] != "window":
            continue
        want = _expected(row, pl, 8)
        got = by_off.get(pl["p"])
        if want == "either":
            continue
        if want is None:
            assert not any(a < pl["p"] + pl["n"] and pl["p"] < b for a, b in covered), (name, pl, "taken beyond a limit")
        else:
            assert got == want, (name, pl, got)
            seen.add((pl["d"], pl["n"]))
    for md, ml, mn, nd in row.props:
        m4 = max(mn, 4)
        assert any(d == md for d, n in seen), (name, "no match at max_dist", md)
        assert any(d == md - 1 for d, n in seen) and not any(d == row.max_dist + 1 for d, n in seen)
        assert (md, m4) in seen, (name, "no match of min_len at the tier's last distance")
        if ml < G.INF and ml <= 0x10000:
            assert (md, ml) in seen, (name, "no match of max_len", ml)
        if md < row.max_dist:                            # one past an inner tier: only with the length the outer tier demands
            outer = min(p[2] for p in row.props if p[0] > md)
            assert (md + 1, max(outer, 4)) in seen or outer > 11
            assert all(n >= outer for d, n in seen if d == md + 1), (name, md + 1)
            assert any(pl["d"] == md + 1 and pl["n"] < outer for pl in plants if pl["kind"] == "window") or outer <= mn
    for s in row.len_steps:
        assert any(n == s for d, n in seen) and any(n == s + 1 for d, n in seen), (name, "length step", s)
    for s in row.dist_steps:
        assert any(d == s for d, n in seen) and any(d == s + 1 for d, n in seen), (name, "distance step", s)
    if row.min_dist > 1:
        assert all(d >= row.min_dist for d, n in by_off.values()), name
    if row.kw.get("strategy", 0) & 1:
        assert all(n <= d for d, n in by_off.values()), name
    # the oracle takes the plants at the limit as well: with fresh bytes in their place the body does not get smaller -- and it stays as it is beyond the limit
    rng = random.Random(7)
    base = len(_oracle_body(oracle, row, data, 8)[0])
    for pl in plants:
        if pl["kind"] == "window" and pl["n"] in (9, 10) and pl["d"] in (row.max_dist - 1, row.max_dist, row.max_dist + 1):
            other = bytearray(data)
            other[pl["p"]:pl["p"] + pl["n"]] = bytes(rng.randrange(256) for _ in range(pl["n"]))
            without = len(_oracle_body(oracle, row, bytes(other), 8)[0])
            if pl["d"] <= row.max_dist:
                assert base < without, (name, pl)
            else:
                assert base == without, (name, pl)


@pytest.mark.parametrize("name", ROW_IDS)
def test_min_len_matches_and_literal_run_steps(name):
    row = G.BY_NAME[name]
    data, plants = G.planted(row)
    if row.min_len < 4:
        by_off = {o: (d, n) for o, d, n in finder_tokens(name, 12) if n}
        assert any(by_off.get(pl["p"]) == (pl["d"], row.min_len) for pl in plants if pl["n"] == row.min_len), (name, "no match of min_len at quality 12")
    toks = finder_tokens(name, 8)
    runs, sp = set(), 0
    for o, d, n in toks:
        runs.add(o - sp); sp = o + n
    for s in row.lit_steps:
        assert s in runs and s + 1 in runs, (name, "literal-run step", s)


def clamp_record(name):
    """{"period:k": [[offset in the run, distance, length], ...]}: the finder's tokens inside each periodic run, at quality 8"""
    row = G.BY_NAME[name]
    _, plants = G.planted(row)
    toks = [t for t in finder_tokens(name, 8) if t[2]]
    out = {}
    for pl in plants:
        if pl["kind"] == "clamp":
            out["%d:%d" % (pl["period"], pl["k"])] = [[o - pl["p"], d, n] for o, d, n in toks if pl["p"] - pl["period"] <= o < pl["p"] + pl["n"]]
    return out


@pytest.mark.parametrize("name", ROW_IDS)
def test_what_follows_a_clamped_match_is_the_committed_list(name):
    row = G.BY_NAME[name]
    want = json.load(open(os.path.join(HERE, "golden", "geometry_clamp.json")))
    got = clamp_record(name)
    assert got == want.get(name, {}), name
    if row.max_len < G.INF:
        assert got and any(any(t[2] == row.max_len for t in v) for v in got.values()), (name, "no run reaches max_len")
