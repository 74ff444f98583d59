"""No GPU: tests/deflate_find_ref.py, the DEFLATE encoder's kernels restated in plain Python, held against everything a CPU can hold it
against -- its `plan` against alz_deflate_plan_block itself (tests/deflate_plan_dump.cpp, the header compiled by g++), its streams against
zlib and the token walker, its matches against an independent brute force, every case of tests/deflate_find_cases.py against the tokens
that prove the case reaches its mechanism, and the bytes of encode() against committed digests.  tests/test_gpu_deflate_find.py then
requires the GPU's bytes to equal encode()'s."""
import functools
import json
import os
import random
import subprocess
import zlib

import pytest

import deflate_find_cases as K
import deflate_find_ref as R
import deflate_walk as W
import test_deflate_cpu as DC
import test_inflate_cpu as IC

ROOT = DC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "deflate_find_vectors.json")
LEVELS = tuple(range(10))


@functools.lru_cache(maxsize=None)
def all_cases():
    return K.synthetic() + K.corpus(K.load_test_bmp())


@functools.lru_cache(maxsize=None)
def tokens(ci, level, k):
    return R.find(all_cases()[ci]["data"], k, level)


@functools.lru_cache(maxsize=None)
def blocks(ci, level, flags):
    return R.blocks(all_cases()[ci]["data"], level, flags, tokens_of=lambda k: tokens(ci, level, k))


# ---------------------------------------------------------------------------------------------- plan against the header itself
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_dump") / "deflate_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(DC.ROCM, "include"), "-I", os.path.join(ROOT, "include"),
                           "-I", DC.CSRC, os.path.join(ROOT, "tests", "deflate_plan_dump.cpp"), "-o", exe])

    def run(records):
        text = "".join("%d %d %d %d %d %s %s\n" % (final, stored_only, fixed_only, raw_len, ntok, " ".join(map(str, lf)), " ".join(map(str, df)))
                       for lf, df, raw_len, ntok, final, stored_only, fixed_only in records)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == len(records)
        return lines
    return run


def plan_line(p):
    return "%d %d %d %d %d %d | %s | %s | %s" % (p["type"], p["bits"], p["bytes"], p["hdr_bits"], p["size"][1], p["size"][2], " ".join(map(str, p["lit_len"])),
                                                 " ".join(map(str, p["dist_len"])), p["hdr"].hex() or "-")


def code_length_code_depth(p):
    """the unlimited depth of the code-length code of a plan's dynamic header"""
    cl_freq = [0] * R.NCL
    for s, _ in R.run_lengths(p["lit_len"], p["dist_len"])[2]:
        cl_freq[s] += 1
    return K.unlimited_depth(cl_freq)


def hold_plans(dump, records, what):
    for i, (rec, line) in enumerate(zip(records, dump(records))):
        assert plan_line(R.plan(*rec)) == line, "%s, record %d: the Python plan and alz_deflate_plan_block differ" % (what, i)


def test_plan_equals_the_header_on_random_and_adversarial_histograms(dump):
    rng = random.Random(21)
    records, cuts15, cuts7 = [], 0, 0

    def add(lf, df, raw_len=None):
        lf = list(lf)
        lf[256] = 1
        for final in (0, 1):
            for fixed_only in (0, 1):
                records.append((lf, list(df), sum(lf) if raw_len is None else raw_len, sum(lf) - 1, final, 0, fixed_only))
    zl, zd = [0] * R.NLIT, [0] * R.NDIST
    add(zl, zd, 0)                                                              # one used symbol; an empty distance set
    add([7 if s == 65 else 0 for s in range(R.NLIT)], zd)                       # one literal and the end
    add([9 if s == 260 else 0 for s in range(R.NLIT)], [9 if s == 5 else 0 for s in range(R.NDIST)])   # one distance symbol
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for n in (17, 20, 22):                                                      # the 15-bit cut
        add([fib[s // 6] if s % 6 == 0 and s // 6 < n else 0 for s in range(R.NLIT)], zd, 30000)
        add([sum(fib[:min(n, 30)]) if s == 257 else 0 for s in range(R.NLIT)], fib[:min(n, 30)] + [0] * (30 - min(n, 30)), 30000)
    add([30000 if s == 101 else 1 for s in range(R.NLIT)], [1] * 29 + [0], 30000)
    # the 7-bit cut: code lengths 1..15 in Fibonacci counts make the code-length code deep
    lf = [0] * R.NLIT
    at = 0
    for depth, count in zip(range(15, 0, -1), (2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)):
        for _ in range(count):
            lf[at] = 1 << (15 - depth)
            at += 3
    add(lf, zd, 30000)
    for rnd in range(2000):
        kind = rnd % 3
        nsym = rng.randrange(1, 286) if kind else rng.randrange(1, 12)
        lf, df = [0] * R.NLIT, [0] * R.NDIST
        for s in rng.sample(range(R.NLIT), nsym):
            lf[s] = 1 + (rng.randrange(40) if kind == 1 else int(rng.paretovariate(0.6)) % 30000 if kind == 2 else rng.randrange(3000))
        nmatch = sum(lf[257:])
        for _ in range(min(nmatch, rng.randrange(1, 31))):
            df[rng.randrange(R.NDIST)] += 1 + (rng.randrange(50) if kind != 2 else int(rng.paretovariate(0.6)) % 5000)
        add(lf, df, rng.randrange(0, 32705))
    for rec in records[::4]:
        p = R.plan(*rec)
        cuts15 += max(p["lit_len"]) == 15 and K.unlimited_depth(rec[0]) > 15
        cuts7 += code_length_code_depth(p) > 7
    assert len(records) >= 4 * 2000 and cuts15 >= 3 and cuts7 >= 3, (cuts15, cuts7)
    hold_plans(dump, records, "histograms")


def test_plan_equals_the_header_on_every_case(dump):
    records = []
    for ci, c in enumerate(all_cases()):
        n = len(c["data"])
        for level in (1, 4, 6, 9):
            for k in range((n + R.BLOCK - 1) // R.BLOCK if n else 1):
                t = tokens(ci, level, k)
                lf, df = R.histograms(t)
                blen = min(n - k * R.BLOCK, R.BLOCK)
                for fixed_only in (0, 1):
                    records.append((lf, df, blen, len(t), int(k * R.BLOCK + blen == n), 0, fixed_only))
    records.append(([0] * 256 + [1] + [0] * 29, [0] * 30, 100, 0, 1, 1, 0))          # level 0: stored only
    hold_plans(dump, records, "cases")


# ---------------------------------------------------------------------------------------------- every stream is valid and says what find and plan said
@pytest.mark.parametrize("level", LEVELS)
def test_streams_are_valid_and_hold_the_tokens_of_find(level):
    from auroralib.compression_amd import _lib
    L = _lib.load()
    for ci, c in enumerate(all_cases()):
        d = c["data"]
        for flags in (0, R.FIXED_FLAG):
            bl = blocks(ci, level, flags)
            s = b"".join(b["bytes"] for b in bl)
            tag = "%s level %d flags %d" % (c["name"], level, flags)
            z = zlib.decompressobj(-15)
            assert z.decompress(s) == d and z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", tag
            assert len(s) <= L.alz_deflate_bound(len(d)) == R.bound(len(d)), tag
            walked, used = W.walk(s)
            assert used == len(s), tag
            # (a block that is not the last and not stored ends with an empty stored block: the walker shows it as a block of its own)
            mine = [w for w in walked if not (w["type"] == W.STORED and w["stored"] == 0 and not w["final"])] if len(d) else walked
            assert len(mine) == len(bl), tag
            for w, b in zip(mine, bl):
                assert (w["type"], w["start"], bool(w["final"])) == (b["plan"]["type"], b["start"], b is bl[-1]), tag
                assert level > 0 or w["type"] == W.STORED, tag
                assert not (flags and w["type"] == W.DYNAMIC), tag
                if w["type"] != W.STORED:
                    assert [t[:3] for t in w["tokens"]] == b["tokens"], tag
        if level:
            bl = blocks(ci, level, 0)
            bad = K.failed_checks(c, level, bl)
            assert not bad, "a case no longer reaches its mechanism: %r" % (bad,)
            # ... and the tokens are in the BYTES the GPU is compared by: a stored block would hide them
            hidden = [pos for levels, pos, _, _, _ in c["checks"] if level in levels and bl[pos // R.BLOCK]["plan"]["type"] == R.STORED]
            assert not hidden, "%s level %d: the block of the checks at %r is stored" % (c["name"], level, hidden)


def test_plan_edges_are_reached():
    by = {c["name"]: i for i, c in enumerate(all_cases())}
    p = blocks(by["stored ties with fixed"], K.TIE_LEVEL, 0)[0]["plan"]
    assert R.block_bytes_of(p["size"][1], True) == p["bytes"] and p["type"] == R.STORED, "the tie goes to the simpler form"
    p = blocks(by["fixed ties with dynamic"], K.TIE_LEVEL, 0)[0]["plan"]
    assert R.block_bytes_of(p["size"][1], True) == R.block_bytes_of(p["size"][2], True) == p["bytes"] and p["type"] == R.FIXEDB
    for name, nlit, ndist in (("one literal", 2, 0), ("no match at all", 5, 0), ("one distance symbol", None, 1)):
        lf, df = R.histograms(blocks(by[name], 6, 0)[0]["tokens"])
        assert (nlit is None or sum(1 for f in lf if f) == nlit) and sum(1 for f in df if f) == ndist, name
    for level in range(1, 10):                     # a dynamic header with an empty distance set
        assert blocks(by["no match at all"], level, 0)[0]["plan"]["type"] == R.DYNAMIC, level
    for level in K.FIB_LEVELS:                     # the Kraft repair of the 15-bit cut runs on the block's own histogram
        b = blocks(by["the 15-bit cut"], level, 0)[1]
        df = R.histograms(b["tokens"])[1]
        assert b["plan"]["type"] == R.DYNAMIC and max(b["plan"]["dist_len"]) == 15 and K.unlimited_depth(df) > 15, (level, [f for f in df if f])


# ---------------------------------------------------------------------------------------------- the restatement against a brute force
def brute_force(d):
    """per position of a one-block input the longest match over ALL earlier positions (the nearest of the longest), at most 258 bytes and
    inside the input; three bytes further than 4 096 back are none.  Earlier positions are looked up by their first three bytes."""
    n, where, out = len(d), {}, []
    for p in range(n):
        best = dist = 0
        maxlen = min(n - p, 258)
        if maxlen >= 3:
            for q in reversed(where.get(d[p:p + 3], ())):
                ln = 0
                while ln < maxlen and d[q + ln] == d[p + ln]:
                    ln += 1
                if ln > best:
                    best, dist = ln, p - q
            where.setdefault(d[p:p + 3], []).append(p)
        if best < 3 or (best == 3 and dist > 4096):
            best = dist = 0
        out.append((best, dist))
    return out


def restated(d, level=9):
    _, best = R.find_all(d, 0, level, every=True)
    return [(best[p][0], best[p][1] if best[p][0] else 0) for p in range(len(d))]


def collision_free(d):
    """no two different trigrams of d in one hash bucket"""
    buckets = {}
    return all(buckets.setdefault(R.trigram_hash(d[p] | (d[p + 1] << 8) | (d[p + 2] << 16)), d[p:p + 3]) == d[p:p + 3] for p in range(len(d) - 2))


def exact_inputs():
    """low-entropy inputs, each the first of its seeds whose trigrams share no bucket (the test proves the preconditions again)"""
    def six(seed):
        rng = random.Random(seed)
        letters = bytes(rng.sample(range(256), 6))
        return bytes(rng.choice(letters) for _ in range(6000))

    def gradient(seed):
        levels = random.Random(seed).sample(range(256), 40)
        return bytes(levels[(i // 200) + (i * i // 977) % 3] for i in range(6000))

    def soup(seed):
        rng = random.Random(seed)
        letters = bytes(rng.sample(range(256), 3))
        words = [bytes(rng.choice(letters) for _ in range(rng.randrange(2, 6))) for _ in range(12)]
        return b"".join(rng.choice(words) for _ in range(1500))[:5000]
    return [(name, next(d for d in map(make, range(400)) if collision_free(d))) for name, make in (("six letters", six), ("gradient", gradient), ("three-letter words", soup))]


def test_level_9_equals_the_brute_force_where_the_chains_are_complete(capsys):
    for name, d in exact_inputs():
        # the preconditions, proven here: one block; no two different trigrams in one bucket; no bucket with more than 1 024 entries
        assert len(d) <= R.BLOCK
        buckets, counts = {}, {}
        for p in range(len(d) - 2):
            t = d[p:p + 3]
            h = R.trigram_hash(t[0] | (t[1] << 8) | (t[2] << 16))
            assert buckets.setdefault(h, t) == t, "%s: two trigrams in bucket %d" % (name, h)
            counts[t] = counts.get(t, 0) + 1
        assert max(counts.values()) <= 1024, name
        want, got = brute_force(d), restated(d)
        share = sum(1 for L, _ in want if L >= 3) / len(d)
        with capsys.disabled():
            print("\n%s: %d bytes, %.3f of the positions have a match of three bytes or more" % (name, len(d), share))
        assert share >= 0.5, name
        assert got == want, "%s: position %d" % (name, next(p for p in range(len(d)) if got[p] != want[p]))


def test_on_text_and_the_bitmap_the_restatement_is_never_longer(capsys):
    bmp = K.load_test_bmp()
    for name, d in (("Test.bmp at 54", bmp[54:54 + 20000]), ("word text", IC.text_like(20000, 7))):
        want, got = brute_force(d), restated(d)
        shorter = sum(1 for g, w in zip(got, want) if g[0] < w[0])
        other = sum(1 for g, w in zip(got, want) if g[0] == w[0] and g != w)
        with capsys.disabled():
            print("\n%s: %d positions, shorter than the brute force at %d (%.4f), another distance at %d (%.4f)" % (name, len(d), shorter, shorter / len(d), other, other / len(d)))
        assert all(g[0] <= w[0] for g, w in zip(got, want)), name


# ---------------------------------------------------------------------------------------------- the committed digests
def test_golden_digests():
    want = json.load(open(GOLDEN))
    index = {c["name"]: ci for ci, c in enumerate(all_cases())}
    got = K.vectors(all_cases(), lambda c, level, flags: b"".join(b["bytes"] for b in blocks(index[c["name"]], level, flags)))
    assert sorted(got) == sorted(want["vectors"])
    bad = [k for k in got if got[k] != want["vectors"][k]]
    assert not bad, "encode() no longer writes the committed bytes: %r" % bad[:5]
