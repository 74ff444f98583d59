#!/usr/bin/env python3
"""make_bitlz_kats.py -- hand-assembled known answers for the CRILAYLA and ALLZ bodies and files (alz_bitlz_*, alz_crilayla_*, alz_allz_*).

This script calls NO decoder, not the library and not tests/bitlz_ref.py: every stream is written down bit by bit next to the C# statement
that reads it (the reference's src/AuroraLib.Compression-Extended/CRI/CRILAYLA.cs and Specialized/ALLZ.cs), and the expected output, status,
dst_len and src_used are written down by hand from those statements.  tests/test_bitlz_cpu.py holds tests/bitlz_ref.py against them and re-runs
this script so the file cannot drift; tests/test_gpu_bitlz.py holds the kernels against them.

Output: tests/golden/bitlz_kat.json (committed).  src_used / dst_len null = unspecified or not written down.

CRILAYLA (CRILAYLA.cs:123-188): GetBits starts at the LAST byte and moves down, MSB first.  The bit strings below are in the order read; they
are packed MSB first into bytes and the bytes are then reversed.  `out` is in MEMORY order: the last byte produced comes first, and the bytes
sit at the top of the span.
  :134  1 bit: 1 = match, 0 = literal (8 bits)
  :136  13 bits + 3 = distance;  :140-148  fields of 2, 3, 5, 8, 8 ... bits, all ones = go on;  length = 3 + their sum
ALLZ (ALLZ.cs:90-127): FlagReader(source, Endian.Little) -- a flag byte is fetched at the current position when a bit is needed and none is
left, bits LSB first; raw run bytes sit at the current position too.  Items below: a bit string (in the order read) or raw bytes.
  :97   1 bit: 0 = a run of ReadALFlag(flags[3]) + 1 raw bytes, 1 = none;  :106-107  distance = ReadALFlag(flags[2]) + 1, length = ReadALFlag(flags[1]) + 3
  :118-126  ReadALFlag(s): 1-bits (each adds one to bits = s), a 0-bit, `bits` bits LSB first, + ((1 << (bits - s)) - 1) << s
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
CASES = []


def case(name, kind, src, out, status, dst_len, src_used, cap=None, decom_len=None, params=None, file=False):
    CASES.append(dict(name=name, kind=kind, file=file, src=src.hex(), cap=cap, decom_len=decom_len, params=params,
                      out=None if out is None else out.hex(), status=status, dst_len=dst_len, src_used=src_used))


def cri_pack(*fields):
    """bit strings in the order read -> the body (zero padding in the final byte)"""
    bits = "".join(fields).replace(" ", "")
    bits += "0" * (-len(bits) % 8)
    return bytes(reversed(bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))))


def allz_pack(*items):
    """bit strings / raw bytes in the order read -> the body: a flag byte is reserved where the first bit of each group of eight is written"""
    out, at, n = bytearray(), None, 0
    for it in items:
        if isinstance(it, bytes):
            out += it
            continue
        for ch in it.replace(" ", ""):
            if at is None or n == 8:
                at, n = len(out), 0
                out.append(0)
            out[at] |= int(ch) << n
            n += 1
    return bytes(out)


# ---------------------------------------------------------------------------------------------- CRILAYLA
CRI1 = cri_pack("0 01000001",                       # literal 'A'
                "0 01000010",                       # literal 'B'
                "0 01000011",                       # literal 'C'
                "1 0000000000000 10",               # match: distance 0 + 3, length 3 + 2 = 5                       -> ABCAB
                "0 01000100",                       # literal 'D'
                "1 0000000000001 11 111 00001")     # match: distance 1 + 3 = 4, length 3 + 3 + 7 + 1 = 14          -> CABDCABDCABDCA
assert CRI1.hex() == "107e0048440070889020"
CRI1_OUT = b"ABCABCAB" + b"D" + b"CABDCABDCABDCA"   # in the order produced
assert len(CRI1_OUT) == 23 and CRI1_OUT[::-1] == b"ACDBACDBACDBACDBACBACBA"
case("crilayla: literals, a match, an overlapping match", "crilayla", CRI1, CRI1_OUT[::-1], OK, 23, 10, cap=64)
case("crilayla: dst_cap inside the last match", "crilayla", CRI1, CRI1_OUT[:22][::-1], CAPACITY, 22, None, cap=22)
# without the byte at the lowest address (the one read last) the final match ends inside its 5-bit field: it produces nothing
case("crilayla: input ends inside the last token", "crilayla", CRI1[1:], b"ABCABCABD"[::-1], TRUNC, 9, 9, cap=64)
assert CRI1[1:].hex() == "7e0048440070889020"
CRI2 = cri_pack("0 01000001", "0 01000010", "1 0000000000000 00")   # 'A', 'B', match(distance 3, length 3) with two bytes produced
assert CRI2.hex() == "0000a09020"
case("crilayla: distance beyond the bytes produced", "crilayla", CRI2, b"BA", BAD, 2, 5, cap=64)
case("crilayla: empty input", "crilayla", b"", b"", OK, 0, 0, cap=16)
# the file: magic, size 23, csize 10, the body, 0x100 plain header bytes -> header bytes, then the 23 bytes at the top of a span of 0x100 + 23
CRI_HDR = bytes(range(256))
CRI_FILE = bytes.fromhex("4352494c41594c41170000000a000000") + CRI1 + CRI_HDR
case("crilayla: the first body as a file", "crilayla", CRI_FILE, CRI_HDR + CRI1_OUT[::-1], OK, 279, 282, file=True)

# ---------------------------------------------------------------------------------------------- ALLZ, (copy, dist, len) = (0, 10, 1)
ALLZ1 = allz_pack("0", "1 0 00", b"ABC",            # run: ReadALFlag(1): bits 2, value 0 + ((1 << 1) - 1) << 1 = 2, + 1 = 3 raw bytes
                  "0 0100000000", "1 0 1",          # distance: bits 10, value 2, + 1 = 3; length: bits 1, value 1 + 1 = 2, + 3 = 5        -> ABCAB
                  "1",                              # no run
                  "0 0000000000", "0",              # distance 0 + 1 = 1; length: bits 0, 0 + 3 = 3                                      -> BBB
                  "0", "0 0", b"D",                 # run: bits 1, value 0, + 1 = 1 raw byte
                  "0 1100000000", "111 0 001")      # distance 3 + 1 = 4; length: bits 3, value 4 + ((1 << 3) - 1) = 11, + 3 = 14         -> BBBDBBBDBBBDBB
assert ALLZ1.hex() == "82414243000d003044c011"
ALLZ1_OUT = b"ABC" + b"ABCAB" + b"BBB" + b"D" + b"BBBDBBBDBBBDBB"
assert ALLZ1_OUT == b"ABCABCABBBBDBBBDBBBDBBBDBB" and len(ALLZ1_OUT) == 26
P = [0, 10, 1]
case("allz: runs, matches, an overlapping match", "allz", ALLZ1, ALLZ1_OUT, OK, 26, 11, cap=26, decom_len=26, params=P)
case("allz: decom_len inside the last match", "allz", ALLZ1, ALLZ1_OUT[:25], MISMATCH, 25, None, cap=25, decom_len=25, params=P)
case("allz: dst_cap below decom_len", "allz", ALLZ1, ALLZ1_OUT[:25], CAPACITY, 25, None, cap=25, decom_len=26, params=P)
case("allz: decom_len beyond what the input holds", "allz", ALLZ1, ALLZ1_OUT, TRUNC, 26, 11, cap=27, decom_len=27, params=P)
for k in range(len(ALLZ1)):                         # every proper prefix ends inside a token or in front of a flag byte the loop still needs
    case("allz: cut to %d bytes" % k, "allz", ALLZ1[:k], None, TRUNC, None, k, cap=26, decom_len=26, params=P)
ALLZ2 = allz_pack("1", "0 0000000000", "0")         # no run; distance 1, length 3 with nothing produced
assert ALLZ2.hex() == "0100"
case("allz: a match as the first token", "allz", ALLZ2, b"", BAD, 0, 2, cap=16, decom_len=16, params=P)
case("allz: decom_len 0", "allz", ALLZ1, b"", OK, 0, 0, cap=0, decom_len=0, params=P)
ALLZ_FILE = bytes.fromhex("414c4c5a00000a011a000000") + ALLZ1
case("allz: the body as a file", "allz", ALLZ_FILE, ALLZ1_OUT, OK, 26, 23, file=True)

if __name__ == "__main__":
    with open(os.path.join(HERE, "bitlz_kat.json"), "w") as fh:
        json.dump({"cases": CASES}, fh, indent=1)
        fh.write("\n")
    print("wrote %d cases" % len(CASES))
