"""The built streams of tests/chunk_phase_cases.py, pinned from the reference side before any GPU sees them: the oracle decodes every assembled body to exactly
the expansion of its token list (status OK, src_used == len(src)); status cases give the status they state.  The recorded marks prove that a case is what its
name says -- output positions, ring offsets, chunk counts of a batch, landing offsets of the walk --, and the tail rule holds: QCH + 76 input bytes (QCH = 1024
at most) lie behind every case, so the lane-parallel rounds, not the exact tail parser, decode it.

Round starts are not observable from outside.  The builders model them as "the byte behind a refused element": a round ends in front of an element it refuses
(ALZ_NX_BAD), the exact parser takes that one element and the next round starts behind it.  This stands in for `adv` of a filler round; the W1 family sweeps ten
neighbouring landing offsets, which keeps it useful if the model is off by a few bytes."""
import pytest

import chunk_phase_cases as CP
import oracle_lib as O
import test_gpu_scalar_paths as SP
from auroralib.compression_amd import _abi as A

PAIRS = [(r, f) for r in CP.ROWS for f in CP.families_of(r)]
POPULATED = [p for p in PAIRS if CP.has_cases(*p)]


def _plain(toks):
    """a token list as test_gpu_scalar_paths.expand takes it: no element breaks, no copy-form field"""
    return [t[:3] for t in toks if t[0] != CP.BREAK]


_cache = {}


def expanded(row_name, family):
    key = (row_name, family)
    if key not in _cache:
        _cache[key] = [CP.expand(toks) for _, toks, _ in CP.cases(row_name, family)]
    return _cache[key]


@pytest.mark.parametrize("row_name,family", PAIRS)
def test_oracle_decodes_every_case_to_its_expansion(row_name, family):
    row = CP.ROWS[row_name]
    for (name, toks, ex), want in zip(CP.cases(row_name, family), expanded(row_name, family)):
        it = CP.item(row, toks, ex, want)
        got, res = O.decode_stream(row.fmt, it["src"], decom_len=it["decom_len"], cap=it["cap"], aux0=it.get("aux0", 0), aux1=it.get("aux1", 0), lz=row.lz)
        if ex.get("status") is not None:
            assert res.status == ex["status"], (row_name, name, res.status)
            assert bytes(got[:res.dst_len]) == want[:res.dst_len], (row_name, name)
            continue
        assert (res.status, res.dst_len, res.src_used) == (A.ST_OK, len(want), len(it["src"]) - row.unread), (row_name, name, res.status, res.dst_len, res.src_used, len(it["src"]))
        assert bytes(got[:len(want)]) == want, (row_name, name)
        assert len(want) <= 24 << 10, (row_name, name, len(want))


@pytest.mark.parametrize("row_name", sorted(CP.ROWS))
def test_the_sliced_expansion_is_the_byte_wise_one(row_name):
    """chunk_phase_cases.expand against test_gpu_scalar_paths.expand: overlapping matches of every small distance, sources in front of the stream start, long tokens"""
    for family in ("C3", "C5", "C6", "W3") if CP.ROWS[row_name] in CP.COPY_ROWS else ("W2", "W3"):
        for (_, toks, _), want in list(zip(CP.cases(row_name, family), expanded(row_name, family)))[:6]:
            assert SP.expand(_plain(toks)) == want, (row_name, family)
    toks = [(SP.LIT, 9), (SP.MATCH, 5, 3)] + [(SP.MATCH, d, n) for d in range(1, 40) for n in (d - 1, d, d + 1, 2 * d + 1, 100) if n > 0]
    assert SP.expand(toks) == CP.expand(toks)


@pytest.mark.parametrize("row_name,family", PAIRS)
def test_tail_rule(row_name, family):
    """QAHEAD_MAX input bytes lie behind the last token of every case (W4 breaks the rule on purpose and says so)"""
    row = CP.ROWS[row_name]
    for name, toks, ex in CP.cases(row_name, family):
        behind = len(row.written(toks)) - len(row.written(toks, ex["case_end"]))
        if ex.get("no_margin"):
            want = ex["marks"][-1]["tail_input"]
            assert behind == ex["marks"][-1]["behind"] and abs(behind - want) <= 3, (row_name, name, behind, want)
            continue
        assert ex["case_end"] > 0 and behind >= CP.QAHEAD_MAX, (row_name, name, behind)


@pytest.mark.parametrize("row_name,family", PAIRS)
def test_marks_say_what_the_case_is(row_name, family):
    row = CP.ROWS[row_name]
    for name, toks, ex in CP.cases(row_name, family):
        for m in ex["marks"]:
            t = toks[m["tok"]] if m["tok"] < len(toks) else None
            pos = sum(1 if x[0] == SP.LIT else x[2] for x in _plain(toks[:m["tok"]]))
            assert pos == m["pos"], (row_name, name)
            if "d" in m:                                 # the match the case is about stands at the mark
                assert t == (SP.MATCH, m["d"], m["n"]), (row_name, name, t, m)
            if "edge" in m:                              # C9: the run's first byte, found in the written body, at that byte of a 512-byte cache chunk
                assert CP.run_offset(row, toks, m) % 512 == m["edge"] % 512, (row_name, name, m)
            if "reach" in m:                             # W1: the element at byte 255 is the row's largest: R literals and a match, in the row's order
                k, R = m["tok"], m["reach"]
                lits = toks[k:k + R] if row_name in CP.LITS_FIRST else toks[k + 1:k + 1 + R]
                assert len(lits) == R and all(x[0] == SP.LIT for x in lits) and toks[k + R if row_name in CP.LITS_FIRST else k][0] == SP.MATCH, (row_name, name, m)
            if "model_target" in m:                      # W1, filler model: the walk restated over the element sizes lands there, and the sizes add up to the written prefix
                sizes = CP.model_sizes(row, toks, m)
                assert CP.walk_model(sizes + [m["m"]])[-1] == m["model_target"], (row_name, name, m)
                assert sum(sizes) == row.size(toks[:m["tok"]]) - row.size(toks[:m["origin"]]), (row_name, name, m)
            if family in ("C1", "C2", "C3") and "d" in m and m["d"] <= m["pos"]:
                assert m["d"] > 2500 and (family == "C3" or m["pos"] >= 4096 + 2560), (row_name, name, m)
            if "fp" in m:                                # C3: the first byte of the chunk's 20-byte read-back
                assert m["fp"] == m["pos"] - m["d"] - (m["pos"] & 3), (row_name, name, m)
            if "ends" in m:                              # C4: the match ends 5 bytes past the ring seam
                assert (m["pos"] + m["n"]) % CP.RING == m["ends"], (row_name, name, m)
            if "off" in m:                               # C7: ring offset of the destination / of the source
                at = m["pos"] - (m["d"] if m["source"] else 0)
                assert (at - m["off"]) % CP.RING == 0 and at >= CP.RING - 20, (row_name, name, m)
            if row.sync is None and ("chunk" in m or "split" in m):
                continue                                 # (a row without a refused element: the place in the step is by chance, NOT_EXPRESSIBLE says so)
            if "chunk" in m and m["chunk"] == 63:        # C1: 63 chunks stand between the round start and the match
                assert _chunks_back(row, toks, m["tok"]) == 63, (row_name, name, m)
            if "chunks" in m or "one_chunk_tokens" in m:  # C8: chunk count of the batch between the mark and its end mark
                end = next(e for e in ex["marks"] if e.get("end") and e["tok"] > m["tok"])
                got = sum(CP.chunks_of(x[1], x[2]) if x[0] == SP.MATCH else 1 for x in _tokens(toks[m["tok"]:end["tok"]]))
                assert got == m.get("chunks", m.get("one_chunk_tokens")), (row_name, name, got, m)
            if "split" in m:                             # C8: the 80-byte token has `first` chunks in the step that the tokens in front of it fill
                assert t[2] == 80 and _chunks_back(row, toks, m["tok"]) == 64 - m["split"][0], (row_name, name, m)
            if "tsm" in m:
                assert m["tsm"] == -(-min(1000, row.max_len) // 3)
            if "target" in m:                            # W1: the landing offset, by writing the two prefixes
                assert CP.landing(row, toks, m) == m["target"] and sum(1 for x in toks[m["round"]:m["tok"]] if x[0] == SP.MATCH) <= 32, (row_name, name, m)
            if "k" in m:                                 # C6: k links of distance n and length n behind the mark
                assert toks[m["tok"]:m["tok"] + m["k"]] == [(SP.MATCH, m["n"], m["n"])] * m["k"], (row_name, name, m)
            if "run" in m:                               # C9: a literal run of that length stands at the mark
                assert all(x[0] == SP.LIT for x in toks[m["tok"]:m["tok"] + m["run"]]) and toks[m["tok"] + m["run"]][0] == SP.MATCH, (row_name, name, m)


def _tokens(toks):
    """literal runs as one token each"""
    out, run = [], 0
    for x in toks:
        if x[0] == SP.LIT:
            run += 1
            continue
        if run:
            out.append((SP.LIT, run)); run = 0
        out.append(x)
    if run:
        out.append((SP.LIT, run))
    return out


def _chunks_back(row, toks, k):
    """chunks between token k and the refused element in front of it (a row without one: the literal run in front of the group)"""
    n, i = 0, k - 1
    while i >= 0 and toks[i][0] == SP.MATCH and toks[i][1] != 1500 and toks[i][1] != 0x20000:
        n += CP.chunks_of(toks[i][1], toks[i][2]); i -= 1
    lits = 0
    while i >= 0 and toks[i][0] == SP.LIT:
        lits += 1; i -= 1
    return n + (1 if 0 < lits < 100 else 0)


@pytest.mark.parametrize("row_name", [r.name for r in CP.COPY_ROWS])
def test_c3_read_back_starts_at_every_offset_around_position_zero(row_name):
    """fp = p - d - b takes every value of -3 .. +3 with the source inside the stream (p >= d): the byte-wise path decides inside one dword"""
    got = {m["fp"] for _, _, ex in CP.cases(row_name, "C3") for m in ex["marks"] if "fp" in m and m["pos"] >= m["d"]}
    assert got >= set(range(-3, 4)), (row_name, sorted(got))


def test_every_row_and_family_is_populated_or_listed():
    for row_name, family in PAIRS:
        assert CP.has_cases(row_name, family) == bool(CP.cases(row_name, family)), (row_name, family)
        if not CP.cases(row_name, family):
            listed = [k for k in CP.NOT_EXPRESSIBLE if k[0] == row_name and k[1] == family]
            assert listed or (family == "C10" and row_name not in CP.C10_ROWS), (row_name, family)
    for (row_name, family, case), why in CP.NOT_EXPRESSIBLE.items():
        assert row_name in CP.ROWS and family in CP.FAMILIES and why, (row_name, family, case)


NOT_EXPRESSIBLE_COUNT = {"lz4_block": 0, "lzo": 3, "snappy_raw": 4, "fastlz": 10, "fastlz_level2": 4, "wflz": 6, "wflz_be": 6, "refpack": 9, "hig": 0,
                        "cns": 1, "cnx2": 2, "lzshrek": 3, "prs_be": 1, "prs_le": 1}


def test_not_expressible_count_per_row():
    CP.build_all()
    got = {r: sum(1 for k in CP.NOT_EXPRESSIBLE if k[0] == r) for r in CP.ROWS}
    assert got == NOT_EXPRESSIBLE_COUNT, got
