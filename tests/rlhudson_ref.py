"""Pure-Python restatement of RLHudson (Hudson Soft's byte RLE, the sibling of RLE30), as the independent check of the alz_rlhudson_* entry
points (the C oracle has no such body).  Line numbers are those of the reference's src/AuroraLib.Compression.Nintendo/HudsonSoft/RLHudson.cs
and src/AuroraLib.Compression/MatchFinder/RleMatchFinder.cs.

The decoder returns (bytes written at dst_off, status, dst_len, src_used); src_used is None where the header leaves it unspecified
(OUTPUT_CAPACITY).  The rules are RLE30's (tests/rlh_ref.py), which is where E5 -- the token that meets dst_cap -- is restated from."""
from rlh_ref import OK, INPUT_TRUNCATED, OUTPUT_SIZE_MISMATCH, OUTPUT_CAPACITY, _rel_match_length

FLAG_MASK, MAX_LENGTH = 0x80, 0x7F                                 # :16-17


def rlhudson_decode(src, decom_len, cap):
    """RLHudson.DecompressHeaderless  :54-81; E5 as RLE30."""
    src = bytes(src)
    out = bytearray()
    p = 0
    while len(out) < decom_len:                                   # :60
        if p >= len(src):                                         # :62 ReadByte() = -1: flag < 0x80, a run of 127 whose ReadUInt8 throws  :67
            return bytes(out), INPUT_TRUNCATED, len(out), len(src)
        flag = src[p]                                             # :62
        length = flag & MAX_LENGTH                                # :63 (may be 0)
        if flag < FLAG_MASK:                                      # :65-68
            if p + 1 >= len(src):                                 # ReadUInt8 throws, also in front of a run of 0
                return bytes(out), INPUT_TRUNCATED, len(out), len(src)
            tok = bytes([src[p + 1]]) * length
            p += 2
        else:                                                     # :69-73 (read into the stack buffer: a short run is never written)
            if p + 1 + length > len(src):
                return bytes(out), INPUT_TRUNCATED, len(out), len(src)
            tok = src[p + 1:p + 1 + length]
            p += 1 + length
        if len(out) + len(tok) > cap:                             # E5: the token that would exceed dst_cap is clipped and ends decoding
            end = len(out) + len(tok)
            out += tok[:cap - len(out)]
            if end > decom_len and cap >= decom_len:
                return bytes(out), OUTPUT_SIZE_MISMATCH, len(out), p
            return bytes(out), OUTPUT_CAPACITY, len(out), None
        out += tok                                                # :74
    if len(out) > decom_len:                                      # :77-80
        return bytes(out), OUTPUT_SIZE_MISMATCH, len(out), p
    return bytes(out), OK, len(out), p


def try_to_find_match(src, p, min_match=3, max_match=MAX_LENGTH):
    """RleMatchFinder(3, 0x7F).TryToFindMatch  RleMatchFinder.cs:29-51 (tests/rlh_ref.py restates it inside rle30_encode): (found, duration),
    defect included -- `duration = source.Length - offset` (:43) lets a literal run reach 128 or 129 bytes."""
    duration = _rel_match_length(src[p:p + min(max_match, len(src) - p)])         # :31-32
    if duration >= min_match:                                                     # :34
        return True, duration                                                     # :50
    duration = 0
    while True:
        duration += 1                                                             # :39
        if len(src) - p - duration < min_match:                                   # :41-45
            return False, len(src) - p
        if duration == max_match or _rel_match_length(src[p + duration:p + duration + min_match]) == min_match:   # :46-47
            return False, duration                                                # :48


def rlhudson_encode(src):
    """RLHudson.CompressHeaderless  :83-102; the over-long literal runs get the control bytes (byte)(duration | 0x80) = 0x80 / 0x81."""
    src = bytes(src)
    out = bytearray()
    p = 0
    while p < len(src):                                                           # :88
        found, duration = try_to_find_match(src, p)                               # :90
        if found:
            out.append(duration & 0xFF)                                           # :92
            out.append(src[p])                                                    # :93
        else:
            out.append((duration | FLAG_MASK) & 0xFF)                             # :97
            out += src[p:p + duration]                                            # :98
        p += duration                                                             # :100
    return bytes(out)


def rlhudson_encode_bound(n):
    """every token spends one control byte on at least one input byte"""
    return 2 * n


def rlhudson_has_defect(src):
    """does the managed encoder write a literal run of 128 or 129 bytes for `src` (a stream that does not decode back)"""
    src, p = bytes(src), 0
    while p < len(src):
        found, duration = try_to_find_match(src, p)
        if not found and duration > MAX_LENGTH:
            return True
        p += duration
    return False
