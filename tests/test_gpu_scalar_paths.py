"""-m gpu: the scalar side of the flag-byte decode -- the real group chain of an iteration (chain_walk_wide, csrc/alz_decode_fast.h) and the loop control of
the byte phase's steady state (byte_emit_steps, csrc/alz_emit_byte.h: a trip of two steps ends a batch, reaches a flush point or wraps the mark tag).

Streams are hand-assembled from token lists by the small encoders below (so that group sizes, batch lengths and flush points are chosen, not found), decoded
through the host-buffer ABI against the oracle (gpu_common.compare_batch: lane-parallel and exact kernels) and through device-resident plans into canary-filled
destinations (test_gpu_canary.canary_decode: kernel variants 1 and 2, and variant 3 -- the work queue of chunks).  The oracle is the reference; the token lists'
own expansion (`expand`) is compared with it as well, so that a slip of an encoder here shows as such.

What a case is for:
  chain         group sizes 9 .. 25 (Yaz0) / 9 .. 33 (LZ11) / 9 .. 17 (LZ10) laid out so that a group starts at byte 63, 64, 65, 127 of an iteration, that the chain
                ends at exactly 128 and beyond it, after 4 .. 8 groups (a group is at most 33 bytes: fewer than 4 cannot fill 128), all-literal and all-longest
                groups alternating, and inputs that END after 1 .. 8 groups
  loop control  batches (64 tokens = one iteration) of every length 0, 1, 63, 64, 65, 127, 128, 129 beyond a multiple of 128; long batches whose flush points fall on
                their first trip, their last trip and between two inner loops; 48 KiB streams of long batches (the mark tag wraps after 255 blocks = 32 640 bytes);
                matches that reach in front of the stream start inside the first 4 KiB, matches that end at exactly 4 096 and 4 097
  shapes        every batch runs as kernel variant 1, 2 and 3; 41 KiB and 90 KiB streams cross the hand-over between chunks in variant 3
  formats       Yay0 / MIO0 (three cursors, descriptor table), LZSS (10, 6, 2) (no table) and LZSS (8, 4, 2) (flush block of 64 bytes: every trip is a flush point)"""
import numpy as np
import pytest

import oracle_lib as O
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import synth
from gpu_common import compare_batch, pack_streams
from test_gpu_canary import canary_decode

pytestmark = pytest.mark.gpu

LIT, MATCH = 0, 1
# longest match of a format's encodings, by token size in bytes
MAXLEN = {A.FMT_YAZ0: 273, A.FMT_LZ10: 18, A.FMT_LZ11: 65808, A.FMT_MIO0: 18, A.FMT_YAY0: 273}


# ------------------------------------------------------------------------------------------------ token lists -> streams
def expand(tokens, window=4096):
    """What a token list decodes to: out[q] = out[q - d], bytes in front of the stream start read as zero (E2)."""
    out = bytearray()
    for t in tokens:
        if t[0] == LIT:
            out.append(t[1])
        else:
            _, d, n = t
            for _ in range(n):
                out.append(out[len(out) - d] if d <= len(out) else 0)
    return bytes(out)


def _match_bytes(fmt, d, n):
    if fmt == A.FMT_YAZ0:
        if n <= 17:
            return bytes([((n - 2) << 4) | ((d - 1) >> 8), (d - 1) & 0xFF])
        return bytes([(d - 1) >> 8, (d - 1) & 0xFF, n - 0x12])
    if fmt in (A.FMT_LZ10, A.FMT_MIO0):
        return bytes([((n - 3) << 4) | ((d - 1) >> 8), (d - 1) & 0xFF])
    if fmt == A.FMT_LZ11:
        if n <= 16:
            return bytes([((n - 1) << 4) | ((d - 1) >> 8), (d - 1) & 0xFF])
        if n <= 272:
            v = n - 17
            return bytes([v >> 4, ((v & 0xF) << 4) | ((d - 1) >> 8), (d - 1) & 0xFF])
        v = n - 273
        return bytes([0x10 | (v >> 12), (v >> 4) & 0xFF, ((v & 0xF) << 4) | ((d - 1) >> 8), (d - 1) & 0xFF])
    raise ValueError(fmt)


def assemble(fmt, tokens, lz=None):
    """The headerless body of `tokens` and the descriptor fields that go with it."""
    if fmt in (A.FMT_YAY0, A.FMT_MIO0):
        flags, codes, lits = bytearray(), bytearray(), bytearray()
        for i in range(0, len(tokens), 8):
            fb = 0
            for k, t in enumerate(tokens[i:i + 8]):
                if t[0] == LIT:
                    fb |= 0x80 >> k
                    lits.append(t[1])
                elif fmt == A.FMT_MIO0 or t[2] <= 17:
                    codes += bytes([((t[2] - (3 if fmt == A.FMT_MIO0 else 2)) << 4) | ((t[1] - 1) >> 8), (t[1] - 1) & 0xFF])
                else:
                    codes += bytes([(t[1] - 1) >> 8, (t[1] - 1) & 0xFF])
                    lits.append(t[2] - 0x12)
            flags.append(fb)
        flags += bytes((-len(flags)) % 4)
        return dict(fmt=fmt, src=bytes(flags + codes + lits), aux0=len(flags), aux1=len(flags) + len(codes))
    body = bytearray()
    pos = 0
    for i in range(0, len(tokens), 8):
        grp = tokens[i:i + 8]
        fb = 0
        data = bytearray()
        for k, t in enumerate(grp):
            if fmt == A.FMT_LZSS:
                if t[0] == LIT:
                    fb |= 1 << k
                    data.append(t[1])
                    pos += 1
                else:
                    off = (pos - t[1] + lz.windows_start) & (lz.max_distance - 1)
                    data += bytes([off & 0xFF, ((off >> 8) << lz.length_bits) | (t[2] - lz.min_length)])
                    pos += t[2]
            else:
                literal_is_one = fmt == A.FMT_YAZ0
                if (t[0] == LIT) == literal_is_one:
                    fb |= 0x80 >> k
                data += bytes([t[1]]) if t[0] == LIT else _match_bytes(fmt, t[1], t[2])
        body.append(fb)
        body += data
    return dict(fmt=fmt, src=bytes(body))


def item(fmt, tokens, lz=None, window=4096, **kw):
    raw = expand(tokens, window)
    it = assemble(fmt, tokens, lz)
    it.update(decom_len=len(raw), cap=len(raw), want=raw, **kw)
    return it


def run(items, what, lz=None, queue=True):
    """Host-buffer ABI against the oracle (both kernel families), the expansion of the token lists against the oracle, then canary-filled device buffers in every kernel shape."""
    streams, src, dst_bytes = pack_streams(items, dst_slack=16)
    gr, g_dst = compare_batch(streams, src, dst_bytes, lz=lz, what=what)
    rec = synth.stream_records(streams)
    for i, it in enumerate(items):
        if it.get("want") is not None and not it.get("cut"):
            a = int(rec["dst_off"][i])
            assert gr["status"][i] == A.ST_OK and gr["dst_len"][i] == len(it["want"]), (what, i, gr["status"][i], gr["dst_len"][i], len(it["want"]))
            assert bytes(g_dst[a:a + len(it["want"])]) == it["want"], (what, i)
    canary_decode(streams, src, dst_bytes, lz=lz, what=what, variants=(1, 2))
    if queue:
        canary_decode(streams, src, dst_bytes, lz=lz, what=what, queue=True)


def _rand_tokens(rng, total, maxdist, minlen, maxlen, p_match=0.45, early=False):
    """Tokens that decode to exactly `total` bytes.  early: distances may reach in front of the stream start (E2)."""
    toks, pos = [], 0
    while pos < total:
        left = total - pos
        if left >= minlen and rng.random() < p_match:
            n = int(min(left, rng.integers(minlen, min(maxlen, 40) + 1) if rng.random() < 0.8 else rng.integers(minlen, maxlen + 1)))
            n = max(n, minlen)
            if n > left:
                n = left
            lim = maxdist if early else max(1, min(maxdist, pos))
            d = int(rng.integers(1, lim + 1)) if rng.random() < 0.7 else int(rng.integers(1, min(lim, 8) + 1))
            if pos == 0 and not early:
                toks.append((LIT, int(rng.integers(0, 256)))); pos += 1
                continue
            toks.append((MATCH, d, n)); pos += n
        else:
            toks.append((LIT, int(rng.integers(0, 256)))); pos += 1
    return toks


# ------------------------------------------------------------------------------------------------ the chain
def _group(fmt, size, rng, pos):
    """Eight tokens whose group takes `size` input bytes (flag byte included): 9 = all literals, 9 + 8 x (longest token - 1) = all longest matches."""
    extra = size - 9
    per = {A.FMT_YAZ0: (2, 1), A.FMT_LZ10: (1,), A.FMT_LZ11: (3, 2, 1)}[fmt]       # input bytes a match token takes beyond a literal's one
    es = []
    for k in range(8):
        e = next((x for x in per if x <= extra), 0)
        es.append(e); extra -= e
    assert extra == 0, size
    rng.shuffle(es)
    toks = []
    for e in es:
        if e == 0:
            toks.append((LIT, int(rng.integers(0, 256)))); pos += 1
        else:                                      # (a match at the very start of a stream reads zeros: E2)
            lo, hi = {A.FMT_YAZ0: {1: (3, 17), 2: (18, 60)}, A.FMT_LZ10: {1: (3, 18)}, A.FMT_LZ11: {1: (3, 16), 2: (17, 60), 3: (273, 300)}}[fmt][e]
            toks.append((MATCH, int(rng.integers(1, min(4096, max(pos, 1)) + 1)), int(rng.integers(lo, hi + 1)))); pos += toks[-1][2]
    return toks, pos


def _stream_of_groups(fmt, sizes, rng):
    toks, pos = [], 0
    for sz in sizes:
        g, pos = _group(fmt, sz, rng, pos)
        toks += g
    return toks


@pytest.mark.parametrize("fmt", [A.FMT_YAZ0, A.FMT_LZ11, A.FMT_LZ10])
def test_chain_lands_on_every_boundary(fmt):
    rng = np.random.default_rng(4100 + fmt)
    big = {A.FMT_YAZ0: 25, A.FMT_LZ11: 33, A.FMT_LZ10: 17}[fmt]
    items = []

    def sizes_to(target):
        """group sizes whose starts run 0, .., target: the chain of the first iteration has a group starting exactly there"""
        out, at = [], 0
        while at < target:
            step = min(big, target - at)
            if 0 < target - at - step < 9:
                step -= 9 - (target - at - step)
            assert step >= 9
            out.append(step); at += step
        return out
    tail = [9, big] * 12
    for lead in ([], [9], [big, 9]):
        for target in (63, 64, 65, 127, 128, 129, 140, 150):
            sz = lead + sizes_to(target - sum(lead))
            if len(sz) > (7 if target < 128 else 8):   # (LZ10's groups are at most 17 bytes: seven of them end at 119, eight at 136)
                continue
            items.append(item(fmt, _stream_of_groups(fmt, sz + tail, rng)))
    # the hop limit: eight short groups end well inside the first 64 bytes / straddle them; all-literal and all-longest groups alternating, both phases
    for sz in ([9] * 40, [big] * 24, [9, big] * 16, [big, 9] * 16, [9, 9, 9, 9, 9, 9, 9, big] * 5, [big, big, big, 9, 9, 9] * 6):
        items.append(item(fmt, _stream_of_groups(fmt, sz, rng)))
    # every group size the format has, at random
    lo_hi = (9, big)
    for _ in range(6):
        items.append(item(fmt, _stream_of_groups(fmt, [int(x) for x in rng.integers(lo_hi[0], lo_hi[1] + 1, 120)], rng)))
    run(items, "chain " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("fmt", [A.FMT_YAZ0, A.FMT_LZ11, A.FMT_LZ10])
def test_input_ends_after_one_to_eight_groups(fmt):
    """The input holds n = 1 .. 8 whole groups (all-literal, all-longest, alternating) and nothing else: the chain walks on into the zero fill behind it, the
    tokens that lie inside the input are a prefix of the lanes.  Also with the declared size beyond what the groups give (the input runs out) and with the
    last group cut in the middle of a token."""
    rng = np.random.default_rng(4200 + fmt)
    big = {A.FMT_YAZ0: 25, A.FMT_LZ11: 33, A.FMT_LZ10: 17}[fmt]
    items = []
    for n in range(1, 9):
        for sz in ([9] * n, [9] + [big] * (n - 1), ([9, big] * 4)[:n], ([9, 9, big] * 3)[:n]):
            it = item(fmt, _stream_of_groups(fmt, sz, rng))
            items.append(it)
            items.append(dict(it, decom_len=it["decom_len"] + 100, cap=it["cap"] + 100, cut=True))
            if len(it["src"]) > 3:
                items.append(dict(it, src=it["src"][:len(it["src"]) - int(rng.integers(1, 4))], cut=True))
    run(items, "ends after n groups " + A.FORMAT_NAMES[fmt])


# ------------------------------------------------------------------------------------------------ loop control of the byte phase
def _batch(rng, T, pos, maxlen=273, minlen=3):
    """64 tokens that decode to T bytes, 64 <= T <= 48 + 16 maxlen.  At most two matches per group: a group is at most 13 input bytes, the eight groups start inside
    the first 92 bytes of an iteration, so ONE iteration (eight hops) takes exactly these 64 tokens -- as long as the stream is made of such batches only."""
    nm = 0 if T == 64 else 1
    while (64 - nm) + nm * maxlen < T:
        nm += 1
    while nm and (64 - nm) + nm * minlen > T:      # (T = 65: no match fits -- unreachable lengths are the caller's to avoid)
        nm -= 1
    assert nm <= 16 and (nm or T == 64), T
    lens, rest = [], T - (64 - nm)
    for i in range(nm):
        later = nm - 1 - i
        n = max(minlen, rest - maxlen * later, min(maxlen, rest - minlen * later, rest // (later + 1) + int(rng.integers(0, 3))))
        lens.append(n); rest -= n
    assert rest == 0 and all(minlen <= n <= maxlen for n in lens), (T, lens)
    slots = [8 * j + k for j in range(8) for k in rng.choice(np.arange(1, 8), 2, replace=False)]
    where = set(int(x) for x in rng.choice(slots, nm, replace=False)) if nm else set()
    toks, li = [], 0
    for k in range(64):
        if k in where:
            d = int(rng.integers(1, min(4096, max(pos, 1)) + 1)) if rng.random() < 0.6 else int(rng.integers(1, min(6, max(pos, 1)) + 1))
            toks.append((MATCH, d, lens[li])); pos += lens[li]; li += 1
        else:
            toks.append((LIT, int(rng.integers(0, 256)))); pos += 1
    return toks, pos


def _stream_of_batches(rng, Ts, lead=4096 + 64):
    """`lead` bytes of short batches (the first W bytes of a stream run unpipelined), then one batch per entry of Ts."""
    toks, pos = [], 0
    while pos < lead:
        b, pos = _batch(rng, int(rng.integers(66, 200)), pos)
        toks += b
    starts = []
    for T in Ts:
        starts.append(pos)
        b, pos = _batch(rng, T, pos)
        toks += b
    return toks, starts


def test_batch_lengths_around_the_trip_size():
    rng = np.random.default_rng(4300)
    items = []
    for m in (0, 1, 2, 3, 9):
        Ts = [128 * m + r for r in (0, 1, 63, 64, 65, 127, 128, 129) if 128 * m + r >= 64 and 128 * m + r != 65]            # (65 = 63 literals + a match of 2: no such match)
        for rep in range(2):
            order = [Ts[i] for i in rng.permutation(len(Ts))]
            toks, _ = _stream_of_batches(rng, order)
            items.append(item(A.FMT_YAZ0, toks, dst_misalign=int(rng.integers(0, 16))))
    toks, _ = _stream_of_batches(rng, [int(x) for x in rng.integers(66, 1400, 60)])
    items.append(item(A.FMT_YAZ0, toks))
    run(items, "batch lengths")


def test_flush_points_on_first_trip_last_trip_and_between_inner_loops():
    """Flush blocks are 1 024 bytes of the destination's 16-byte-aligned coordinates.  `gap` bytes in front of a flush point a long batch starts: gap <= 128 puts
    the flush on its first trip; a batch of gap + 0 .. 127 bytes more than whole trips puts it on the last; 2 500 .. 4 000 bytes cross two to four flush
    points, each between two inner loops."""
    rng = np.random.default_rng(4400)
    items = []
    for mis in (0, 5, 15):
        for gap in (1, 64, 127, 128, 129, 300, 1024):
            for T in (gap, gap + 127, 128 * ((gap + 127) // 128), 1024 + gap, 2500, 4000):
                if T < 64:
                    continue
                # bring the output position to (flush point - gap) with one adjusting batch
                toks, pos = [], 0
                while pos < 4096 + 200:
                    b, pos = _batch(rng, int(rng.integers(66, 200)), pos); toks += b
                adj = (-(pos + mis) - gap) % 1024
                if adj < 66:
                    adj += 1024
                b, pos = _batch(rng, adj, pos); toks += b
                assert (pos + mis + gap) % 1024 == 0
                for TT in (T, 640, T):
                    b, pos = _batch(rng, TT, pos); toks += b
                items.append(item(A.FMT_YAZ0, toks, dst_misalign=mis))
    run(items, "flush points")


@pytest.mark.parametrize("fmt", [A.FMT_YAZ0, A.FMT_LZ10])
def test_48k_streams_cross_the_tag_wrap(fmt):
    """The mark tag runs 1 .. 255, one per block of 128 bytes: it wraps after 32 640 bytes of blocks (per stream in variants 1 / 2, per 40 KiB chunk in variant 3).
    Long batches (the wrap falls inside a steady state), short ones (the wrap falls on an unpipelined step) and a mix."""
    rng = np.random.default_rng(4500 + fmt)
    maxlen = MAXLEN[fmt]
    items = []
    top = 48 + 16 * maxlen                                             # the longest batch of 64 tokens _batch makes
    for lo, hi in ((top - top // 4, top), (66, 200), (66, top // 2)):
        for rep in range(3):
            toks, pos = [], 0
            while pos < 48 * 1024:
                b, pos = _batch(rng, int(rng.integers(lo, hi)), pos, maxlen=maxlen); toks += b
            items.append(item(fmt, toks, dst_misalign=int(rng.integers(0, 16))))
    run(items, "tag wrap " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("fmt", [A.FMT_YAZ0, A.FMT_LZ10, A.FMT_LZ11])
def test_matches_before_the_stream_start_and_ending_at_the_window_size(fmt):
    rng = np.random.default_rng(4600 + fmt)
    maxlen = min(MAXLEN[fmt], 300)
    items = []
    for end in (4096, 4097):
        for rep in range(4):
            toks = _rand_tokens(rng, end - 40 - rep, 4096, 3, maxlen, early=True)
            pos = end - 40 - rep
            n = min(maxlen, 17 + rep)                                  # the match that ENDS at `end`; literals in front of it
            while pos < end - n:
                toks.append((LIT, int(rng.integers(0, 256)))); pos += 1
            toks.append((MATCH, (4096, 1, 4095, 64)[rep], n)); pos += n
            assert pos == end
            toks += _rand_tokens(rng, 3000, 4096, 3, maxlen, early=True)
            items.append(item(fmt, toks))
    for rep in range(4):                                               # far matches only, from the first token on
        items.append(item(fmt, _rand_tokens(rng, 6000, 4096, 3, maxlen, p_match=0.7, early=True)))
    run(items, "early matches " + A.FORMAT_NAMES[fmt])


# ------------------------------------------------------------------------------------------------ kernel shapes and the other byte-phase formats
@pytest.mark.parametrize("fmt", [A.FMT_YAZ0, A.FMT_LZ11])
def test_41k_and_90k_streams_through_the_chunk_hand_over(fmt):
    rng = np.random.default_rng(4700 + fmt)
    items = []
    for total in (41 * 1024, 90 * 1024, 41 * 1024 + 1, 90 * 1024 - 63):
        items.append(item(fmt, _rand_tokens(rng, total, 4096, 3, min(MAXLEN[fmt], 400)), dst_misalign=int(rng.integers(0, 16))))
    toks, pos = [], 0
    while pos < 90 * 1024:
        b, pos = _batch(rng, int(rng.integers(66, 1500)), pos); toks += b
    items.append(item(fmt, toks))
    run(items, "chunk hand-over " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("fmt", [A.FMT_YAY0, A.FMT_MIO0])
def test_three_cursor_formats(fmt):
    rng = np.random.default_rng(4800 + fmt)
    items = [item(fmt, _rand_tokens(rng, total, 4096, 3, MAXLEN[fmt], early=e)) for total, e in ((1, False), (4096, True), (4097, True), (9000, False), (41 * 1024 + 5, False), (50000, True))]
    run(items, "three cursors " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("bits", [(10, 6, 2), (8, 4, 2)])
def test_lzss_geometries(bits):
    """(10, 6, 2): a 1 KiB window, flush blocks of 256 bytes, no descriptor table.  (8, 4, 2): a 256-byte window whose flush block is 64 bytes -- less than one trip of
    the steady state, so every trip is a flush point."""
    lz = A.LzProperties.from_bits(*bits)
    W, maxlen = 1 << bits[0], (1 << bits[1]) - 1 + 3
    rng = np.random.default_rng(4900 + bits[0])
    items = []
    for total, e in ((1, False), (W, True), (W + 1, True), (5000, False), (20000, True), (41 * 1024 + 7, False)):
        items.append(item(A.FMT_LZSS, _rand_tokens(rng, total, W, 3, maxlen, early=e), lz=lz, window=W, dst_misalign=int(rng.integers(0, 16))))
    toks, pos = [], 0
    while pos < 12000:                                                 # batches of 64 tokens of chosen lengths
        b, pos = _batch(rng, int(rng.integers(66, 48 + 16 * maxlen)), pos, maxlen=maxlen)
        toks += [(t[0], min(t[1], W), t[2]) if t[0] == MATCH else t for t in b]
    items.append(item(A.FMT_LZSS, toks, lz=lz, window=W))
    run(items, "lzss %r" % (bits,), lz=lz)
