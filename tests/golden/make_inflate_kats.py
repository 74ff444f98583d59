#!/usr/bin/env python3
"""make_inflate_kats.py -- hand-assembled known answers for raw DEFLATE streams (alz_inflate_*).

This script calls NO decoder, not the library, not tests/inflate_ref.py and not zlib: every stream is written down bit by bit from RFC 1951,
and the expected output, status, dst_len and src_used are written down by hand from the frozen rules of include/auroralz.h.
tests/test_inflate_cpu.py holds tests/inflate_ref.py against them and re-runs this script so the file cannot drift; tests/test_gpu_inflate.py
holds the kernels against them.

Output: tests/golden/inflate_kat.json (committed).  src_used null = unspecified.

Bit strings below are in the order READ: the first character is bit 0 of byte 0 (DEFLATE packs LSB first).  A Huffman code is written as in
the RFC (its first bit first); an integer field is written through v(value, nbits), least significant bit first.
  header      BFINAL, then BTYPE as v(type, 2): stored "00", fixed "10", dynamic "01", type 3 "11"
  fixed code  literal 0..143: 8 bits, 00110000 + value; 144..255: 9 bits; 256..279: 7 bits, 0000000 + (symbol - 256); 280..287: 8 bits,
              11000000 + (symbol - 280); distance symbols: 5 bits
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
CASES = []


def case(name, src, out, status, src_used, cap=64):
    CASES.append(dict(name=name, src=src.hex(), cap=cap, out=out.hex(), status=status, dst_len=len(out), src_used=src_used))


def v(value, nbits):
    return "".join(str((value >> i) & 1) for i in range(nbits))


def pack(*items, pad="0"):
    """bit strings (in the order read) and raw bytes (at a byte boundary) -> the stream; `pad` fills the last byte"""
    out, bits = bytearray(), ""
    for it in items:
        if isinstance(it, bytes):
            assert not bits
            out += it
            continue
        bits += it.replace(" ", "")
        while len(bits) >= 8:
            out.append(int(bits[7::-1], 2))
            bits = bits[8:]
    if bits:
        bits += pad * (8 - len(bits))
        out.append(int(bits[::-1], 2))
    return bytes(out)


def lit8(ch):
    """the fixed code of a literal below 144"""
    return format(0x30 + ord(ch), "08b")


# ---------------------------------------------------------------------------------------------- fixed blocks
F1 = ("1 10",                                    # BFINAL, fixed
      lit8("a"), lit8("b"), lit8("c"),           # 10010001 10010010 10010011
      "0000001",                                 # symbol 257: length 3, no extra bits
      "00010",                                   # distance symbol 2: distance 3
      "0000000")                                 # end of block -- 3 + 24 + 7 + 5 + 7 = 46 bits
assert lit8("a") == "10010001" and sum(len(x.replace(" ", "")) for x in F1) == 46
FIXED1 = pack(*F1)
assert len(FIXED1) == 6
case("fixed: three literals, a match, end of block", FIXED1, b"abcabc", OK, 6)
case("fixed: the padding of the last byte is ones", pack(*F1, pad="1"), b"abcabc", OK, 6)
case("fixed: trailing bytes are not consumed", FIXED1 + b"\x00\xff", b"abcabc", OK, 6)
case("fixed: dst_cap inside the match", FIXED1, b"abca", CAPACITY, None, cap=4)
case("fixed: dst_cap at the literals' end, the match does not fit", FIXED1, b"abc", CAPACITY, None, cap=3)
case("fixed: dst_cap exact", FIXED1, b"abcabc", OK, 6, cap=6)
case("fixed: dst_cap 0", FIXED1, b"", CAPACITY, None, cap=0)
# 5 bytes = 40 bits: the match (bits 27..38) is whole, the end-of-block code (39..45) is cut
case("fixed: cut inside the end-of-block code", FIXED1[:5], b"abcabc", TRUNC, 5)
# 4 bytes = 32 bits: the length code (27..33) is cut; a match is one symbol
case("fixed: cut inside the match", FIXED1[:4], b"abc", TRUNC, 4)
case("fixed: cut to one byte", FIXED1[:1], b"", TRUNC, 1)
case("empty input", b"", b"", TRUNC, 0)
case("fixed: an empty final block", pack("1 10", "0000000"), b"", OK, 2)
case("fixed: literal/length symbol 286", pack("1 10", lit8("a"), "11000110"), b"a", BAD, None)
case("fixed: distance symbol 30", pack("1 10", lit8("a"), "0000001", "11110"), b"a", BAD, None)
case("fixed: distance 2 with one byte produced", pack("1 10", lit8("a"), "0000001", "00001", "0000000"), b"a", BAD, None)
case("fixed: distance 2 with two bytes produced", pack("1 10", lit8("a"), lit8("b"), "0000001", "00001", "0000000"), b"ababa", OK, 5)
# symbol 285 (8 bits: 11000000 + 5) is length 258 without extra bits; distance symbol 0 is distance 1
case("fixed: length 258 at distance 1", pack("1 10", lit8("z"), "11000101", "00000", "0000000"), b"z" * 259, OK, 4, cap=300)   # 3 + 8 + 8 + 5 + 7 = 31 bits
case("block type 3", pack("1 11"), b"", BAD, None)

# ---------------------------------------------------------------------------------------------- stored blocks
# a stored block that is not the last one, five padding bits of ones, then an empty fixed block
STORED1 = pack("0 00", "11111", b"\x02\x00\xfd\xff", b"hi", "1 10", "0000000")
assert len(STORED1) == 9
case("stored: two bytes, then an empty fixed block", STORED1, b"hi", OK, 9)
case("stored: NLEN is not the complement", pack("1 00", "00000", b"\x02\x00\xfd\xfe", b"hi"), b"", BAD, None)
case("stored: LEN 0 in the final block", pack("1 00", "00000", b"\x00\x00\xff\xff"), b"", OK, 5)
case("stored: the input holds one of three bytes", pack("1 00", "00000", b"\x03\x00\xfc\xff", b"x"), b"x", TRUNC, 6)
case("stored: cut inside NLEN", pack("1 00", "00000", b"\x03\x00\xfc"), b"", TRUNC, 4)
case("stored: dst_cap inside the run", pack("1 00", "00000", b"\x03\x00\xfc\xff", b"xyz"), b"xy", CAPACITY, None, cap=2)

# ---------------------------------------------------------------------------------------------- dynamic blocks
# Literal 'a' (97) and end-of-block (256) with 1-bit codes, no distance code.  HLIT 0 (257 lengths), HDIST 0 (1 length, 0).
# The 258 lengths: 97 zeros, 1, 158 zeros, 1, 0  =  18(97) 1 18(138) 18(20) 1 0  in code-length symbols.
# Code-length code: symbol 1 -> 1 bit "0"; symbol 0 -> 2 bits "10"; symbol 18 -> 2 bits "11" (canonical: 1/2 + 1/4 + 1/4).
# HCLEN order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15: symbol 1 is the 18th, so 18 lengths are written (HCLEN = 14).
CLL = {18: 2, 0: 2, 1: 1}
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
D_HEAD = ("1 01", v(0, 5), v(0, 5), v(14, 4)) + tuple(v(CLL.get(s, 0), 3) for s in ORDER[:18])
D_LENS = ("11" + v(97 - 11, 7), "0", "11" + v(138 - 11, 7), "11" + v(20 - 11, 7), "0", "10")
assert 97 + 1 + 138 + 20 + 1 + 1 == 258
# data: 'a' is the code "0", end of block "1"
DYN1 = pack(*D_HEAD, *D_LENS, "0 0 0", "1")
assert len(DYN1) == 14                           # 3 + 14 + 54 + 9 + 1 + 9 + 9 + 1 + 2 + 4 = 106 bits
case("dynamic: two 1-bit codes, no distance code", DYN1, b"aaa", OK, 14)
case("dynamic: dst_cap 2", DYN1, b"aa", CAPACITY, None, cap=2)
case("dynamic: cut inside the lengths", DYN1[:10], b"", TRUNC, 10)
# the same lengths without the code for 256: 97 zeros, 1, 160 zeros = 18(97) 1 18(138) 18(22)
case("dynamic: no code for end of block", pack(*D_HEAD, "11" + v(86, 7), "0", "11" + v(127, 7), "11" + v(11, 7)), b"", BAD, None)
# 97 + 1 + 138 + 21 = 257 lengths, then a repeat of 21 where one length is left
case("dynamic: a repeat runs past the last length", pack(*D_HEAD, "11" + v(86, 7), "0", "11" + v(127, 7), "11" + v(10, 7), "11" + v(21 - 11, 7)), b"", BAD, None)
# code-length code: 16 -> "0", 18 -> "1" (HCLEN 0: the lengths of 16 17 18 0 are 1 0 1 0); the first symbol is a repeat of nothing
case("dynamic: repeat code 16 with no previous length", pack("1 01", v(0, 5), v(0, 5), v(0, 4), v(1, 3), v(0, 3), v(1, 3), v(0, 3), "0", v(0, 2)), b"", BAD, None)
# 16 -> 1 bit and nothing else: an incomplete code-length code
case("dynamic: an incomplete code-length code", pack("1 01", v(0, 5), v(0, 5), v(0, 4), v(1, 3), v(0, 3), v(0, 3), v(0, 3)), b"", BAD, None)
# 16, 17, 18 -> 1 bit each: over-subscribed
case("dynamic: an over-subscribed code-length code", pack("1 01", v(0, 5), v(0, 5), v(0, 4), v(1, 3), v(1, 3), v(1, 3), v(0, 3)), b"", BAD, None)
case("dynamic: HLIT 30 (287 lengths)", pack("1 01", v(30, 5), v(0, 5), v(0, 4), "0" * 40), b"", BAD, None)
case("dynamic: HDIST 30 (31 lengths)", pack("1 01", v(0, 5), v(30, 5), v(0, 4), "0" * 40), b"", BAD, None)

if __name__ == "__main__":
    with open(os.path.join(HERE, "inflate_kat.json"), "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")
    print("%d cases" % len(CASES))
