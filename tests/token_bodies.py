"""Token list -> headerless body, for every format of the main codec: the writers behind the hand-assembled streams of tests/test_gpu_geometry_edges.py,
tests/chunk_phase_cases.py and their CPU files.  A token list is that of tests/test_gpu_scalar_paths.py: (LIT, byte) and (MATCH, distance, length); `expand` there
says what it decodes to.  Every writer cites the lines of the reference's reader it is read back by."""
import test_gpu_scalar_paths as SP
from auroralib.compression_amd import _abi as A

LIT, MATCH = SP.LIT, SP.MATCH
BREAK = 2                                                # (BREAK,): an element boundary for the writers that can say it (raw Snappy; CNS: an empty literal run)


def _lz40_body(tokens):                                  # LZ40.cs:72-118: flag bits MSB first, negated; u16 LE distance << 4 | length
    body = bytearray()
    for i in range(0, len(tokens), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 8]):
            if t[0] == LIT:
                data.append(t[1])
                continue
            fb |= 0x80 >> k
            _, d, n = t
            if n < 16:
                data += ((d << 4) | n).to_bytes(2, "little")
            elif n < 272:
                data += (d << 4).to_bytes(2, "little") + bytes([n - 16])
            else:
                data += ((d << 4) | 1).to_bytes(2, "little") + (n - 272).to_bytes(2, "little")
        body.append((-fb) & 0xFF)
        body += data
    return bytes(body)


def _flag8_body(tokens, match_bytes, msb=True):
    body = bytearray()
    for i in range(0, len(tokens), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 8]):
            if t[0] == LIT:
                data.append(t[1])
            else:
                fb |= (0x80 >> k) if msb else (1 << k)
                data += match_bytes(t[1], t[2])
        body.append(fb)
        body += data
    return bytes(body)


def _clz0(d, n):                                         # CLZ0.cs:99-130
    delta = 0x1000 - d
    return bytes([delta & 0xFF, (n - 3) | ((delta >> 8) << 4)])


def _seq_body(fmt, tokens):
    """LZ4 blocks (LZ4.cs:202-238), raw Snappy (Snappy.cs:124-203) and CNS (CNS.cs:111-141) from a token list"""
    out, lits = bytearray(), bytearray()
    total = len(SP.expand([t[:3] for t in tokens if t[0] != BREAK]))
    if fmt == A.FMT_SNAPPY_RAW:
        v = total
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80); v >>= 7
        out.append(v)

    def ext(v):
        v -= 15
        b = bytearray()
        if v >= 0:
            while True:
                x = min(v, 255); b.append(x); v -= x
                if x != 255:
                    return b
        return b

    def flush_lits():
        if fmt == A.FMT_SNAPPY_RAW and lits:
            n = len(lits)
            out.extend(bytes([(n - 1) << 2]) if n <= 60 else bytes([60 << 2, n - 1]) if n <= 256 else bytes([61 << 2]) + (n - 1).to_bytes(2, "little"))
            out.extend(lits)
        if fmt == A.FMT_CNS:
            for i in range(0, len(lits), 127):
                out.append(len(lits[i:i + 127])); out.extend(lits[i:i + 127])
        del lits[:]
    for t in tokens + [None]:
        if t is not None and t[0] == LIT:
            lits.append(t[1])
            continue
        if t is not None and t[0] == BREAK and fmt != A.FMT_LZ4_BLOCK:
            # Snappy: the literals so far are an element of their own (two literal elements may stand side by side, Snappy.cs:221-233).  CNS: the same, and one
            # length byte of 0 behind them -- an empty literal copy, which the reader takes and which produces nothing (CNS.cs:89-96)
            flush_lits()
            if fmt == A.FMT_CNS:
                out.append(0)
            continue
        if fmt == A.FMT_LZ4_BLOCK:
            n = t[2] - 4 if t else 0
            out.append((min(len(lits), 15) << 4) | min(n, 15))
            out += ext(len(lits)) + lits
            del lits[:]
            if t:
                out += t[1].to_bytes(2, "little") + ext(n)
            continue
        flush_lits()
        if t is None:
            break
        d, n = t[1], t[2]
        if fmt == A.FMT_SNAPPY_RAW and len(t) > 3 and t[3] == "copy4":       # a fourth token field names the copy form: 4-byte offset  Snappy.cs:245-248
            out += bytes([3 | ((n - 1) << 2)]) + d.to_bytes(4, "little")
        elif fmt == A.FMT_SNAPPY_RAW:
            out += bytes([2 | ((n - 1) << 2)]) + d.to_bytes(2, "little")
        else:
            out += bytes([0x80 | (n - 3), d - 1])
    return bytes(out)


def _lz02(d, n):                                         # LZ02.cs:133-146
    return bytes([((d >> 8) << 4) | (n - 1 if n <= 16 else 0), d & 0xFF]) + (bytes([n - 17]) if n > 16 else b"")


def _lz02_body(tokens):
    """the tokens, then the terminator: a match token of distance 0  LZ02.cs:147-149"""
    body = bytearray()
    toks = tokens + [None]
    for i in range(0, len(toks), 8):
        fb, data = 0, bytearray()
        for k, t in enumerate(toks[i:i + 8]):
            if t is not None and t[0] == LIT:
                data.append(t[1])
            else:
                fb |= 0x80 >> k
                data += bytes(2) if t is None else _lz02(t[1], t[2])
        body.append(fb)
        body += data
    return bytes(body)


def _runs(tokens):
    """[(literals in front, match or None)]"""
    out, lits = [], bytearray()
    for t in tokens:
        if t[0] == LIT:
            lits.append(t[1])
        else:
            out.append((bytes(lits), t)); lits = bytearray()
    out.append((bytes(lits), None))
    return out


def _wflz_body(tokens, big):
    """WFLZ.cs:161-196: blocks of distance (u16), length - 4, literal count, literals; a block without a match carries literals only; four zero bytes end the stream"""
    out = bytearray()
    pending = (0, 0)
    for lits, m in _runs(tokens):
        first = True
        while first or lits:
            d, n = pending
            out += d.to_bytes(2, "big" if big else "little") + bytes([n - 4 if n else 0, min(len(lits), 255)]) + lits[:255]
            lits, pending, first = lits[255:], (0, 0), False
        if m is not None:
            pending = (m[1], m[2])
    if pending != (0, 0):
        out += pending[0].to_bytes(2, "big" if big else "little") + bytes([pending[1] - 4, 0])
    return bytes(out + bytes(4))


def _refpack_body(tokens):
    """RefPack.cs:241-303 through the writer that pins the finder restatement (tests/test_bitenc_cpu.py: refpack_write): the canonical form of every token"""
    from test_bitenc_cpu import refpack_write
    raw, ms, pos = SP.expand(tokens), [], 0
    for t in tokens:
        if t[0] == MATCH:
            ms.append((pos, t[1], t[2]))
        pos += 1 if t[0] == LIT else t[2]
    return refpack_write(raw, ms + [(len(raw), 0, 0)])


def _yay0_token(d, n, extra):                            # Yay0.cs:165-177: lengths from 18 on put a byte into the literal stream
    if n < 18:
        return (((n - 2) << 12) | (d - 1)).to_bytes(2, "big")
    extra.append(n - 0x12)
    return (d - 1).to_bytes(2, "big")


def _lzhudson_body(tokens):
    """Yaz0's tokens under flag words of 32 bits, big-endian, first token in the top bit, 1 = literal  LZHudson.cs:55-59"""
    body = bytearray()
    for i in range(0, len(tokens), 32):
        fw, data = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 32]):
            if t[0] == LIT:
                fw |= 0x80000000 >> k
                data.append(t[1])
            else:
                extra = []
                data += _yay0_token(t[1], t[2], extra) + bytes(extra)
        body += fw.to_bytes(4, "big") + data
    return bytes(body)


def _smsr00_item(tokens):
    """SMSR00.cs:85-131: a section of 16-bit big-endian words -- a mask (first token in the top bit, 1 = literal), then the match words of its 16 tokens -- and the
    literals behind it; aux0 = the length of the first section"""
    codes, lits = bytearray(), bytearray()
    for i in range(0, len(tokens), 16):
        mask, words = 0, bytearray()
        for k, t in enumerate(tokens[i:i + 16]):
            if t[0] == LIT:
                mask |= 0x8000 >> k
                lits.append(t[1])
            else:
                words += (((t[2] - 3) << 12) | (t[1] - 1)).to_bytes(2, "big")
        codes += mask.to_bytes(2, "big") + words
    return dict(fmt=A.FMT_SMSR00, src=bytes(codes + lits), aux0=len(codes), aux1=0)


def _prs_body(tokens, big):
    """PRS.cs:104-159 with the reference's FlagWriter (tests/chain_finder_ref.py): short form for lengths 2..5 at distances up to 0x100, else the long form"""
    from chain_finder_ref import FlagWriter
    fw = FlagWriter(big)
    order = "big" if big else "little"
    for t in tokens:
        if t[0] == LIT:
            fw.buffer.append(t[1]); fw.write_bit(1)
            continue
        _, d, n = t
        fw.write_bit(0)
        if d <= 0x100 and n <= 5:
            fw.write_bit(0); fw.write_bit(((n - 2) >> 1) & 1); fw.write_bit((n - 2) & 1)
            fw.buffer.append((-d) & 0xFF)
            fw.flush_if_necessary()
        else:
            v = ((-d) << 3) & 0xFFFF
            fw.buffer += (v | (n - 2 if n <= 9 else 0)).to_bytes(2, order) + (bytes([n - 1]) if n > 9 else b"")
            fw.write_bit(1)
    fw.write_bit(0); fw.buffer += bytes(2); fw.write_bit(1)
    fw.flush()
    return bytes(fw.out)


def _cnx2_body(tokens):
    """CNX2.cs:140-172: two flag bits per element, least significant first: 01 one literal, 11 a counted run, 10 a match"""
    from chain_finder_ref import FlagWriter
    fw = FlagWriter(False)
    for lits, m in _runs(tokens):
        while lits:
            c = lits[:255]
            if len(c) == 1:
                fw.buffer.append(c[0]); fw.write_bit(1); fw.write_bit(0)
            else:
                fw.buffer.append(len(c)); fw.buffer += c; fw.write_bit(1); fw.write_bit(1)
            lits = lits[255:]
        if m is not None:
            fw.buffer += ((((m[1] - 1) & 0x7FF) << 5) | ((m[2] - 4) & 0x1F)).to_bytes(2, "big")
            fw.write_bit(0); fw.write_bit(1)
    fw.flush()
    return bytes(fw.out)


def _blz_token(d, n):                                    # BLZ.cs:97-135 in stream order: distance - 3 in twelve bits
    return (((n - 3) << 12) | (d - 3)).to_bytes(2, "big")


def _fastlz_body(tokens, level2):
    """FastLZ.cs:162-245: literal runs of at most 32; the level rides on the first byte, which is a literal run's"""
    out, first = bytearray(), level2
    for lits, m in _runs(tokens):
        while lits:
            c = lits[:32]
            out.append((len(c) - 1) | (0x20 if first else 0)); out += c
            first, lits = False, lits[32:]
        if m is None:
            continue
        length, distance = m[2] - 3, m[1] - 1
        short = min(distance, 0x1FFF) if level2 else distance
        out.append(((min(length, 6) + 1) << 5) | (short >> 8))
        if length >= 6:
            length -= 6
            while level2 and length >= 255:
                out.append(255); length -= 255
            out.append(length)
        out.append(short & 0xFF)
        if level2 and distance >= 0x1FFF:
            out += (distance - 0x1FFF).to_bytes(2, "big")
    return bytes(out)


def _shrek_field(v, at):
    return (v, b"") if v < at else (0x1E, bytes([v - at])) if v < at + 256 else (0x1F, (v - at - 256).to_bytes(2, "little"))


def _lzshrek_body(tokens):
    """LZShrek.cs:121-174: a group = literal count field << 3 | matches - 1, the literals, up to eight matches; four zero bytes end the stream"""
    out = bytearray()
    runs = _runs(tokens)
    i = 0
    while i < len(runs):
        lits, m = runs[i]
        group = bytearray()
        count = 0
        while m is not None:
            _, d, n = m
            df, dx = _shrek_field(d - 1, 30)
            group += bytes([(df << 3) | (n if n <= 7 else 0)]) + (bytes([n - 7]) if n > 7 else b"") + dx
            count += 1
            if count == 8 or i + 1 >= len(runs) or runs[i + 1][0] or runs[i + 1][1] is None:
                break
            i += 1
            m = runs[i][1]
        i += 1
        if m is None and not lits:
            break
        uf, ux = _shrek_field(len(lits), 30)
        out += bytes([(uf << 3) | max(count - 1, 0)]) + ux + lits + group
    return bytes(out + bytes(4))


def _hig_raw(lits):                                      # HIG.cs:234-243: count - 2 in a byte (3..257), else 0 and the count as a ushort
    return (bytes([len(lits) - 2]) if 3 <= len(lits) <= 257 else bytes([0]) + len(lits).to_bytes(2, "little")) + lits


def _hig_body(tokens):
    """HIG.cs:214-323: an initial literal block, then matches whose two low bits say what follows: 3 nothing, 1 / 2 that many literals, 0 a literal block"""
    runs = _runs(tokens)
    out = bytearray(_hig_raw(runs[0][0]))
    for k, (_, m) in enumerate(runs):
        if m is None:
            break
        _, d, n = m
        follow = runs[k + 1][0]
        code = 3 if not follow else len(follow) if len(follow) < 3 else 0
        if d <= 0x7FF and n <= 9:
            out.append(code | ((n - 4) << 5) | ((d >> 6) & 0x1C))
        else:
            if d <= 0x3FFF and n <= 35:
                out.append(0xC0 | (n - 4))
            else:
                out.append(0xE0 | ((d >> 10) & 0x10) | (n - 3 if n <= 18 else 0))
                if n > 18:
                    out += bytes([n - 18]) if n <= 273 else bytes([0]) + n.to_bytes(2, "big")
            out.append(code | ((d >> 6) & 0xFC))
        out.append(d & 0xFF)
        out += _hig_raw(follow) if code == 0 else follow
    return bytes(out)


def _lzo_ext(v):                                         # LZO.cs:263-271
    out = bytearray()
    while v > 255:
        out.append(0); v -= 255
    return bytes(out + bytes([v]))


def _lzo_body(tokens):
    """LZO.cs:49-139 read backwards: literal runs of 1..3 ride in the two low bits of the match in front (or, at the start, in a first byte of 17 + count), longer runs
    have an instruction of their own; M2 for lengths up to 8 at distances up to 2048, M3 up to 16384, M4 beyond; 11 00 00 ends the stream"""
    runs = _runs(tokens)
    out = bytearray()
    first = runs[0][0]
    if 0 < len(first) <= 238:
        out += bytes([17 + len(first)]) + first
    for k, (lits, m) in enumerate(runs):
        if k and len(lits) > 3 or not k and len(lits) > 238:
            out += (bytes([len(lits) - 3]) if len(lits) <= 18 else bytes([0]) + _lzo_ext(len(lits) - 18)) + lits
        if m is None:
            break
        _, d, n = m
        follow = runs[k + 1][0]
        p = len(follow) if len(follow) <= 3 else 0
        if n <= 8 and d <= 2048:
            out.append(p | (((d - 1) & 7) << 2) | ((0x40 | ((n - 3) << 5)) if n <= 4 else (0x80 | ((n - 5) << 5))))
            out.append((d - 1) >> 3)
        elif d <= 16384:
            out += bytes([0x20 | (n - 2)]) if n <= 33 else bytes([0x20]) + _lzo_ext(n - 33)
            out += bytes([p | (((d - 1) << 2) & 0xFF), (d - 1) >> 6])
        else:
            dd = d - 0x4000
            flag = 0x10 | ((dd & 0x4000) >> 11)
            out += bytes([flag | (n - 2)]) if n <= 9 else bytes([flag]) + _lzo_ext(n - 9)
            out += bytes([p | ((dd << 2) & 0xFF), (dd >> 6) & 0xFF])
        if p:
            out += follow
    return bytes(out + b"\x11\x00\x00")


EDGE_FORMATS = {
    # name: (format, window, min_len, max_len, body(tokens) -> bytes or None for test_gpu_scalar_paths.assemble, lz)
    "lzss_12_4_2": (A.FMT_LZSS, 0x1000, 3, 18, None, A.LzProperties.from_bits(12, 4, 2)),
    "lzss_10_6_2": (A.FMT_LZSS, 0x400, 3, 66, None, A.LzProperties.from_bits(10, 6, 2)),      # (distance and length bits fill the token's 16: wider geometries have no body to assemble)
    "lzss_8_4_2": (A.FMT_LZSS, 0x100, 3, 18, None, A.LzProperties.from_bits(8, 4, 2)),
    "lz10": (A.FMT_LZ10, 0x1000, 3, 18, None, None),
    "lz11": (A.FMT_LZ11, 0x1000, 3, 0x4000, None, None),
    "yaz0": (A.FMT_YAZ0, 0x1000, 3, 273, None, None),
    "yay0": (A.FMT_YAY0, 0x1000, 3, 273, None, None),
    "mio0": (A.FMT_MIO0, 0x1000, 3, 18, None, None),
    "lz40": (A.FMT_LZ40, 0xFFF, 3, 0x4000, _lz40_body, None),                 # (12 distance bits, no bias: 0xFFF is the farthest a token can say)
    "clz0": (A.FMT_CLZ0, 0x1000, 3, 18, lambda t: _flag8_body(t, _clz0, msb=False), None),
    "lz4_block": (A.FMT_LZ4_BLOCK, 0xFFFF, 4, 100000, lambda t: _seq_body(A.FMT_LZ4_BLOCK, t), None),
    "snappy_raw": (A.FMT_SNAPPY_RAW, 0x8000, 4, 64, lambda t: _seq_body(A.FMT_SNAPPY_RAW, t), None),
    "cns": (A.FMT_CNS, 0x100, 3, 130, lambda t: _seq_body(A.FMT_CNS, t), None),
    "lz02": (A.FMT_LZ02, 0xFFF, 3, 272, _lz02_body, None),
    "wflz": (A.FMT_WFLZ, 0xFFFF, 5, 255, lambda t: _wflz_body(t, False), None),
    "wflz_be": (A.FMT_WFLZ_BE, 0xFFFF, 5, 255, lambda t: _wflz_body(t, True), None),
    "refpack": (A.FMT_REFPACK, 0x20000, 5, 1028, _refpack_body, None),
    "lzhudson": (A.FMT_LZHUDSON, 0x1000, 3, 273, _lzhudson_body, None),
    "smsr00": (A.FMT_SMSR00, 0x1000, 3, 18, _smsr00_item, None),
    # (PRS: a length of 2 exists in the short form only, distances up to 0x100 -- the long form's length field 0 announces a length byte, PRS.cs:83-90: 3 is the
    # shortest match at distance W)
    "prs_be": (A.FMT_PRS_BE, 0x1FFF, 3, 256, lambda t: _prs_body(t, True), None),
    "prs_le": (A.FMT_PRS_LE, 0x1FFF, 3, 256, lambda t: _prs_body(t, False), None),
    "cnx2": (A.FMT_CNX2, 0x800, 4, 35, _cnx2_body, None),
    "blz": (A.FMT_BLZ, 0x1002, 3, 18, lambda t: _flag8_body(t, _blz_token), None),       # (distance - 3 in twelve bits: 0x1002 is the farthest a token can say)
    "fastlz": (A.FMT_FASTLZ, 0x2000, 3, 264, lambda t: _fastlz_body(t, False), None),
    "fastlz_level2": (A.FMT_FASTLZ, 0x11FFF, 3, 100000, lambda t: _fastlz_body(t, True), None),
    "lzshrek": (A.FMT_LZSHREK, 0x1000, 3, 262, _lzshrek_body, None),
    "hig": (A.FMT_HIG, 0x7FFF, 4, 0xFFFF, _hig_body, None),
    "lzo": (A.FMT_LZO, 0xBFFF, 3, 100000, _lzo_body, None),
}


assert sorted({v[0] for v in EDGE_FORMATS.values()}) == list(range(A.FMT_COUNT))       # every body of the main codec


# formats whose first byte is a literal run's (WFLZ: a first block without literals and without a match is the end block, WFLZ.cs:130-159; FastLZ: the level rides on the
# first literal run, FastLZ.cs:181-198; LZO: a first byte above 17 is a literal count, LZO.cs:59-64, and the far match's opcode at distance W is 0x18 and more): no
# stream of theirs starts with a match
FIRST_IS_LITERAL = (A.FMT_WFLZ, A.FMT_WFLZ_BE, A.FMT_FASTLZ, A.FMT_LZO)
