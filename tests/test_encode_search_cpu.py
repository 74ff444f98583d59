"""No GPU: the inputs of tests/encode_search_cases.py prove themselves, from the reference side alone.  For every case, in both variants (dense and lane side):

  * the Python finder is pinned on it: the tokens of chain_finder_ref.matches written through the row's writer (tests/token_bodies.py) are the oracle's bytes;
  * the claim is re-derived: the chain at the proving position P -- every earlier position whose four bytes hash like P's at the quality's hash width, nearest
    first -- is the stated list with the stated number of common bytes; no token of the reference covers P (the cursor, or its lazy step, stands on it); and the
    token the reference writes at P is what MatchSearch restated for ONE position (encode_search_cases.pick) gives from that chain -- the long candidate of K4
    with maxChain - 1 candidates in front of it and not with maxChain, the nearer of two equal candidates, the full length beyond kernel B's cap;
  * the restated probe (enc_probe_kernel: encode_search_cases.probe_counts) puts the variant on its side with the margin the file promises: at most 1 / 8 of the
    samples hit on the dense side, at least 1 / 2 on the lane side; the K6 streams stand on their stated side, the line streams exactly on tot / 4 and around it.

tests/golden/encode_search_digests.json (make_encode_search_digests.py) holds a digest of every (row, quality, family): a change of a builder is noticed.
NOT_EXPRESSIBLE is pinned per row and family below."""
import collections
import functools
import hashlib
import json
import os

import pytest

import chain_finder_ref as CF
import encode_search_cases as ES
import geometry_cases as G
import test_gpu_scalar_paths as SP
import token_bodies as TB

HERE = os.path.dirname(os.path.abspath(__file__))
PAIRS = ES.PAIRS
LIT, MATCH = SP.LIT, SP.MATCH


@pytest.fixture(scope="module")
def oracle():
    import oracle_lib as O
    return O


def finder_body(name, raw, q):
    """(the body the row's writer makes of the finder's tokens, the match list)"""
    row = G.BY_NAME[name]
    data = raw[:len(raw) - ES.tail_skip(row)]
    ms = CF.matches(row.finder_props(), data, q, **row.finder_kw())
    toks, sp = [], 0
    for o, d, n in ms:
        toks += [(LIT, b) for b in data[sp:o]]
        if n == 0:
            break
        toks.append((MATCH, d, n)); sp = o + n
    toks += [(LIT, b) for b in raw[len(data):]]
    fmt, _, _, _, body, lz = TB.EDGE_FORMATS[ES.ROWS[name]]
    return (SP.assemble(fmt, toks, lz)["src"] if body is None else body(toks)), ms


def snappy_write(raw, match_list):
    """Snappy.CompressHeaderless as a function of the match list (Snappy.cs:124-203): the length as a varint; a literal run's length in the tag up to 60, in one or
    two bytes behind it above; a copy with a 1-byte offset for lengths 4 .. 11 at distances below 2 048, with a 2-byte offset otherwise"""
    out, sp, v = bytearray(), 0, len(raw)
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80); v >>= 7
    out.append(v)
    for offset, distance, length in match_list:
        plain = offset - sp
        if plain > 0:
            out += bytes([(plain - 1) << 2]) if plain <= 60 else bytes([60 << 2, plain - 1]) if plain <= 256 else bytes([61 << 2]) + (plain - 1).to_bytes(2, "little")
            out += raw[sp:offset]
            sp = offset
        if length == 0:
            break
        sp += length
        if distance < 2048 and 4 <= length <= 11:
            out += bytes([1 | ((length - 4) << 2) | ((distance >> 8) << 5), distance & 0xFF])
        else:
            out += bytes([2 | ((length - 1) << 2)]) + distance.to_bytes(2, "little")
    return bytes(out)


def check_case(name, q, case, lane, oracle):
    row, f = G.BY_NAME[name], ES.finder(name, q)
    raw, p = case.buffer(lane)
    tag = (name, q, case.name, "lane" if lane else "dense")
    body, ms = finder_body(name, raw, q)
    want = oracle.encode_stream(row.fmt, raw, quality=q, **row.kw)[0]
    if name == "snappy_raw":                             # (the writer of token_bodies says every match as a 2-byte-offset copy: the reference's choice of form is restated above)
        body = snappy_write(raw, ms)
    assert body == want, tag
    data = raw[:len(raw) - ES.tail_skip(row)]
    n = len(data)
    chain = ES.chain_at(data, p, f.hash_bits)
    if case.cands is not None:
        shift = p - case.p
        assert chain == [c + shift for c, _ in case.cands], tag
        assert [ES.common(data, p, c, n - p) for c in chain] == [min(ln, n - p) for _, ln in case.cands], tag
    else:
        assert chain and p - chain[0] == case.claim["first"], tag
    assert not any(o < p < o + ln for o, _, ln in ms), tag + ("a token covers P",)
    d, ln = ES.pick(name, q, data, p)
    at_p = [m for m in ms if m[0] == p and m[2]]
    assert at_p == ([(p, d, ln)] if ln >= f.min_len else []), tag + (at_p, d, ln)
    if "found" in case.claim:                            # K4: the long candidate is the LAST of the chain
        assert (bool(at_p) and at_p[0][1] == p - chain[-1]) == case.claim["found"], tag
    if case.claim.get("lazy"):                           # P - 1 has a match of its own, shorter than P's: the lazy step (LzChainMatchFinder.cs:175-190)
        d1, l1 = ES.pick(name, q, data, p - 1)
        assert f.min_len <= l1 <= f.lazy and l1 < ln and not any(m[0] == p - 1 and m[2] for m in ms), tag
    if "collide" in case.claim:                          # N: P's 15-bit chain meets the collisions first, then the chain at the finder's width
        c15 = ES.chain_at(data, p, 15)
        k = case.claim["collide"]
        assert c15[k] == chain[0] and all(p - c < 24 + 8 * k for c in c15[:k]) and set(chain) <= set(c15), tag   # (further back the background may collide too)
    if "also" in case.claim:
        p2, d2 = case.claim["also"]
        assert [m[1] for m in ms if m[0] == p2 + p - case.p] == [d2], tag
    base = p - case.claim.get("lane", 0)                 # the proving wavefront / block
    found = ES.lane_classes(data, base, f.hash_bits)
    if "classes" in case.claim:                          # K1: the lanes of each stated distance, and no other distance on 8 lanes or more
        assert {d: found.get(d, 0) for d in case.claim["classes"]} == case.claim["classes"], tag + (found,)
        assert all(k < 8 for d, k in found.items() if d not in case.claim["classes"]), tag + (found,)
    if "class_of" in case.claim:
        assert found.get(case.claim["class_of"][0], 0) == case.claim["class_of"][1] >= 8, tag + (found,)
    if "pairs" in case.claim:                            # K5: the pairs of the block of 64 positions (maxChain 4); the blocks of 256 overflow the list of 256 many times
        if f.max_chain == 4:
            assert ES.block_pairs(name, q, data, base, 64) == case.claim["pairs"][f.min_dist], tag
        elif f.max_chain >= 8:
            assert ES.block_pairs(name, q, data, base, 256) > 2 * 256, tag
    if "pairs_dyn" in case.claim:                        # K5: one pair more than the list of 256 holds, in the block of 256 positions
        assert f.max_chain == 16 and ES.block_pairs(name, q, data, base, 256) == case.claim["pairs_dyn"] == 257, tag
    hit, tot = ES.probe_counts(name, q, raw)
    assert tot >= 1024 and (hit * 2 >= tot if lane else hit * 8 <= tot), tag + (hit, tot)
    assert ES.lane_side(hit, tot) == lane, tag
    assert p % 64 == case.p % 64 and len(raw) >= 8192, tag


@pytest.mark.parametrize("name,q", PAIRS)
def test_every_case_proves_itself(name, q, oracle):
    cases = ES.all_cases(name, q)
    assert len(cases) >= (50 if len(ES.families_of(name, q)) > 1 else 3)
    for case in cases:
        for lane in (False, True):
            check_case(name, q, case, lane, oracle)
    # the proving wavefront or block starts at a multiple of 256 (the stream start case: of 64)
    assert all((c.p - c.claim.get("lane", 0)) % 256 == 0 or c.start for c in cases)


def test_a_broken_builder_is_noticed(oracle):
    """one candidate fewer in front of the long one, and the claim `not found` no longer holds; a byte changed behind P, and the stated common length does not"""
    name, q = "yaz0", 3
    case = next(c for c in ES.cases(name, q, "K4") if c.claim.get("found") is False)
    raw = bytearray(case.data)
    c0 = case.cands[0][0]
    raw[c0] ^= 0x40                                     # the nearest candidate leaves the class
    broken = ES.Case(case.name, bytes(raw), case.p, case.cands[1:], claim=case.claim)
    with pytest.raises(AssertionError):
        check_case(name, q, broken, False, oracle)
    case = ES.cases(name, q, "K3")[0]
    raw = bytearray(case.data)
    raw[case.p + 20] ^= 0x40
    with pytest.raises(AssertionError):
        check_case(name, q, ES.Case(case.name, bytes(raw), case.p, case.cands, claim=case.claim), False, oracle)


def test_k6_streams_stand_on_their_side(oracle):
    batch = ES.probe_batch()
    assert sum(1 for _, side in batch if side is True) >= 600 and sum(1 for _, side in batch if side is False) >= 50
    for name, q in (("yaz0", 3), ("yaz0", 8), ("lz10", 12), ("lz10_vram", 8)):
        row = G.BY_NAME[name]
        for i, (raw, side) in enumerate(batch):
            hit, tot = ES.probe_counts(name, q, raw)
            if side is None:
                assert tot == 0 and len(raw) - 4 == 63, i    # limit 63: the probe answers 0 without looking
                continue
            assert tot == len(raw) - 3 and (hit * 2 >= tot if side else hit * 8 <= tot), (name, q, i, hit, tot)
        for raw, _ in batch[::37] + batch[-4:]:
            assert finder_body(name, raw, q)[0] == oracle.encode_stream(row.fmt, raw, quality=q, **row.kw)[0], (name, q)
        for raw, hits in ES.probe_line():
            assert ES.probe_counts(name, q, raw) == (hits, 1024), (name, q, hits)
            assert finder_body(name, raw, q)[0] == oracle.encode_stream(row.fmt, raw, quality=q, **row.kw)[0], (name, q)
    assert [h for _, h in ES.probe_line()] == [256, 255, 257, 254]
    assert [ES.lane_side(h, 1024) for _, h in ES.probe_line()] == [True, False, True, False]


def test_k7_streams_stand_on_their_side_of_the_words_choice(oracle):
    """at most 1 / 16 distinct hashes in the streams of two byte values, at least 14 / 16 in the others: far from 4 / 16 and from 11 / 16"""
    b = ES.words_batches()
    assert len(b["split"]) == 2048 + 64 and 1536 <= min(map(len, b["split"])) and max(map(len, b["split"])) < 3072
    for name, q in ES.WORDS_PAIRS:
        row, inverted = G.BY_NAME[name], name == "yaz0"
        for key in ("split", "few", "many", "collide"):
            sides = []
            for i, raw in enumerate(b[key]):
                fresh, tot, narrow = ES.words_counts(name, q, raw)
                few = ES.few_words(raw)
                assert tot >= 1024 and (fresh * 16 <= tot if few else fresh * 16 >= tot * 14), (name, q, key, i, fresh, tot)
                assert narrow == (few != inverted), (name, q, key, i)
                sides.append(narrow)
            assert sum(sides) == {"split": 1056, "few": 40 if inverted else 60, "many": 60 if inverted else 40, "collide": 40 if inverted else 60}[key], (name, key)
        raw = b["collide"][0]                           # a position whose nearest 15-bit candidate is not on its chain at the finder's width
        bits = ES.finder(name, q).hash_bits
        assert any(ES.chain_at(raw, p, 15)[0] != ES.chain_at(raw, p, bits)[0] for p in range(400, 480, 4)), name
        got = [ES.words_counts(name, q, raw) for raw in b["short"]]
        assert all(not nar for _, t, nar in got if t < 256) and any(t < 256 for _, t, _ in got) and any(t >= 256 for _, t, _ in got), (name, got)
        for raw in b["split"][::96] + b["few"][::25] + b["collide"][::20] + b["short"]:
            assert finder_body(name, raw, q)[0] == oracle.encode_stream(row.fmt, raw, quality=q, **row.kw)[0], (name, q, len(raw))
    src = open(os.path.join(os.path.dirname(HERE), "auroralib", "compression_amd", "csrc", "alz_encode.hip")).read()
    for text in ("#define ALZ_NARROW_SPLIT_MIN 2048u", "#define ALZ_NARROW_MIN_THRESH16 11u", "#define ALZ_NARROW_THRESH16 4u", "const bool narrow = cnt[1] >= 256u && (invert ? !few : few);"):
        assert text in src, text


def test_the_restated_numbers():
    """maxChain, lazy, hash width and kernel B's cap of the four qualities: what the families are built around"""
    f = {q: ES.finder("yaz0", q) for q in ES.QUALITIES}
    assert [(f[q].max_chain, f[q].lazy, f[q].hash_bits) for q in ES.QUALITIES] == [(2, 3, 16), (4, 4, 17), (16, 5, 19), (128, 7, 19)]
    assert [f[q].min_table is not None for q in ES.QUALITIES] == [False, False, False, True]
    caps = {name: [ES.b_cap(G.BY_NAME[name], q) for q in ES.QUALITIES] for name in ES.ROWS}
    assert caps["yaz0"] == caps["lz11"] == caps["lz4_block"] == caps["refpack"] == [48, 48, 256, 48]
    assert caps["lz10"] == caps["lz10_vram"] == caps["lzss_12_4_2_compat"] == [None] * 4
    src = open(os.path.join(os.path.dirname(HERE), "auroralib", "compression_amd", "csrc", "alz_encode.hip")).read()
    for text in ("#define ALZ_PROBE_THRESH16 4u", "#define ALZ_DENSE_LIST 256", "#define ALZ_LEN_CAP 2040", "if (g.max_len < 96) return ALZ_LEN_CAP;",
                 "(g.max_chain <= 5 || g.max_chain >= 64) ? 48 : 256", "while (__popcll(todo) >= 8)", "cmp_max <= 448", "const bool chk = ok && best_l >= 16;",
                 "if (limit < 64) { if (lane == 0) sel[sid] = 0u; return; }", "const bool dyn = g.max_chain >= 8;"):
        assert text in src, text


# ------------------------------------------------------------------------------------------------ what cannot be said, and the digests
NOT_EXPRESSIBLE_COUNTS = {                            # entries over the qualities of a row
    ("yaz0", "K2"): 13, ("yaz0", "K3"): 6, ("yaz0", "K5"): 3, ("yaz0", "S"): 11,
    ("lz10", "K1"): 4, ("lz10", "K2"): 13, ("lz10", "K3"): 4, ("lz10", "K5"): 3, ("lz10", "S"): 11,
    ("lz11", "K2"): 16, ("lz11", "K3"): 6, ("lz11", "K5"): 3, ("lz11", "S"): 11,
    ("lz4_block", "K2"): 16, ("lz4_block", "K3"): 6, ("lz4_block", "K4"): 4, ("lz4_block", "K5"): 3, ("lz4_block", "N"): 4, ("lz4_block", "S"): 12,
    ("lzss_12_4_2_compat", "K1"): 4, ("lzss_12_4_2_compat", "K2"): 13, ("lzss_12_4_2_compat", "K3"): 4, ("lzss_12_4_2_compat", "K5"): 3, ("lzss_12_4_2_compat", "S"): 11,
    ("lz10_vram", "K1"): 4, ("lz10_vram", "K2"): 13, ("lz10_vram", "K3"): 4, ("lz10_vram", "K4"): 2, ("lz10_vram", "K5"): 7, ("lz10_vram", "S"): 11,
    ("refpack", "K2"): 16, ("refpack", "K3"): 6, ("refpack", "K4"): 4, ("refpack", "K5"): 3, ("refpack", "N"): 4,
    ("snappy_raw", "S"): 12,
}


def test_not_expressible_is_pinned():
    table = ES.build_all()
    got = collections.Counter((name, fam) for name, _, fam, _ in table)
    assert dict(got) == NOT_EXPRESSIBLE_COUNTS
    assert all(len(why) > 20 for why in table.values())


@functools.lru_cache(maxsize=None)
def digests():
    out = {}
    for name, q in PAIRS:
        for fam in ES.families_of(name, q):
            h = hashlib.sha256()
            for c in ES.cases(name, q, fam):
                h.update(("%s|%d|%r|%r|" % (c.name, c.p, c.cands, sorted(c.claim.items()))).encode())
                h.update(c.data)
            out["%s q%d %s" % (name, q, fam)] = "%d:%s" % (len(ES.cases(name, q, fam)), h.hexdigest()[:24])
    h = hashlib.sha256()
    for raw, side in ES.probe_batch() + ES.probe_line():
        h.update(raw + repr(side).encode())
    for key, raws in sorted(ES.words_batches().items()):
        for raw in raws:
            h.update(raw)
    out["K6"] = "%d:%s" % (len(ES.probe_batch()) + len(ES.probe_line()), h.hexdigest()[:24])
    return out


def test_golden_digests():
    with open(os.path.join(HERE, "golden", "encode_search_digests.json")) as fh:
        assert digests() == json.load(fh)
