#!/usr/bin/env python3
"""make_kats_rlh.py -- hand-assembled known answers for the RLE30 and HUF20 bodies (alz_rlh_*).

This script calls NO decoder, not the library and not tests/rlh_ref.py: every stream is written down byte by byte next to the C# statement
that reads it (paths under the reference's src/AuroraLib.Compression.Nintendo/Nintendo), and the expected output, status, dst_len and src_used
are written down by hand from those statements.  tests/test_rlh_cpu.py holds tests/rlh_ref.py against them and re-runs this script so the file
cannot drift; tests/test_gpu_rlh.py holds both kernel families against them.

Output: tests/golden/rlh_kat.json (committed; not kat_<name>.json: tests/test_kat.py takes every file of that pattern for an oracle format).  src_used null = unspecified (OUTPUT_CAPACITY, include/auroralz.h).
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OK, TRUNC, MISMATCH, CAPACITY = 0, 1, 2, 3
RLE30, HUF4, HUF8 = 0, 1, 2
CASES = []


def case(name, fmt, src, decom_len, out, status, dst_len, src_used, cap=None, aux0=0):
    out = bytes(out)
    assert len(out) == dst_len
    CASES.append(dict(name=name, fmt=fmt, aux0=aux0, src=bytes(src).hex(), decom_len=decom_len, cap=decom_len if cap is None else cap,
                      out=out.hex(), status=status, dst_len=dst_len, src_used=src_used))


# ------------------------------------------------------------------------------------------------ RLE30  (RLE30.cs:76-105)
# flag = ReadByte(); length = (flag & 0x7F) + 1  (:84-85)
# flag >= 0x80: section = length + 2 bytes filled with ReadUInt8()  (:87-91)  -> control 0x80 | (run - 3), then the byte
# else        : section = length bytes read from the source         (:92-97)  -> control (count - 1), then the bytes
def run(n, b):
    assert 3 <= n <= 130
    return bytes([0x80 | (n - 3), b])


def lit(data):
    assert 1 <= len(data) <= 128
    return bytes([len(data) - 1]) + bytes(data)


case("rle30 run of 3 (shortest)", RLE30, run(3, 0x41), 3, b"AAA", OK, 3, 2)
case("rle30 run of 130 (longest: control 0xFF)", RLE30, run(130, 0x42), 130, b"B" * 130, OK, 130, 2)
case("rle30 literal run of 1 (control 0x00)", RLE30, lit(b"C"), 1, b"C", OK, 1, 2)
case("rle30 literal run of 128 (control 0x7F)", RLE30, lit(bytes(range(128))), 128, bytes(range(128)), OK, 128, 129)
case("rle30 literals, run, literals", RLE30, lit(b"abc") + run(5, 0x78) + lit(b"yz"), 10, b"abcxxxxxyz", OK, 10, 9)
case("rle30 bytes behind the last token are not read", RLE30, run(3, 0x41) + b"\xff\x00", 3, b"AAA", OK, 3, 2)
# the loop runs while Position < endPosition (:82): the last token may overshoot, its bytes are written, then :101-104 throws
case("rle30 overshoot of the declared size", RLE30, run(5, 0x78), 3, b"xxxxx", MISMATCH, 5, 2, cap=8)
case("rle30 overshoot clipped by dst_cap (E4 over E5)", RLE30, run(5, 0x78), 3, b"xxx", MISMATCH, 3, 2, cap=3)
case("rle30 token beyond dst_cap (E5)", RLE30, lit(b"ab") + run(5, 0x78), 7, b"abxx", CAPACITY, 4, None, cap=4)
case("rle30 dst_cap 0", RLE30, run(3, 0x41), 3, b"", CAPACITY, 0, None, cap=0)
# ReadByte() at the end gives -1: a literal run of 128 whose Read comes back short (:84-96)
case("rle30 input ends at a control byte", RLE30, run(3, 0x41), 6, b"AAA", TRUNC, 3, 2)
# ReadUInt8() throws (:90)
case("rle30 input ends at a run byte", RLE30, lit(b"a") + b"\x85", 10, b"a", TRUNC, 1, 3)
# source.Read(section) != length (:95-96): the short run was read into the temporary and is never written
case("rle30 input ends inside a literal run", RLE30, run(3, 0x41) + b"\x03ab", 10, b"AAA", TRUNC, 3, 5)
case("rle30 empty input", RLE30, b"", 4, b"", TRUNC, 0, 0)
case("rle30 decom_len 0 reads nothing", RLE30, run(3, 0x41), 0, b"", OK, 0, 0)
case("rle30 decom_len 0, empty input", RLE30, b"", 0, b"", OK, 0, 0)


# ------------------------------------------------------------------------------------------------ HUF20  (HUF20.cs:94-152)
# byte 0 treeSize, byte 1 treeRoot, treeSize * 2 tree bytes (:98-101); then ReadInt32() words, bit 31 first (:128, :133).
# A node byte: bits 0..5 offset, bit 7 "the left child (bit 0) is a leaf", bit 6 "the right child (bit 1) is a leaf" (:134: leaf =
# treePos >> (5 + direction), direction = 2 - bit).  Its two children are the byte pair at next - 2 / next - 1 with
# next += (offset << 1) + 2 (:132, :136): pair (index of the parent's pair + 1 + offset); the root's pair is pair `offset`.
def words(bits):
    """a string of '0' / '1' -> little-endian 32-bit words consumed MSB first, the last one padded with zeros"""
    bits += "0" * (-len(bits) % 32)
    return b"".join(int(bits[k:k + 32], 2).to_bytes(4, "little") for k in range(0, len(bits), 32))


def tree3(a, b, c):
    """three leaves: a = '0', b = '10', c = '11'.  root (pair 0, left leaf) = 0x80; pair 0 = [a, node]; node (pair 1 = 0 + 1 + offset 0, both
    leaves) = 0xC0; pair 1 = [b, c]"""
    return bytes([2, 0x80, a, 0xC0, b, c])


A_, B_, C_ = "0", "10", "11"
T8 = tree3(0x41, 0x42, 0x43)
case("huf20 8-bit, three leaves", HUF8, T8 + words(A_ + B_ + C_ + A_ + C_ + B_ + A_ + A_), 8, b"ABCACBAA", OK, 8, 10)
case("huf20 8-bit, bits behind the last symbol and bytes behind the last word are not read", HUF8, T8 + words(B_ + "1111") + b"\xaa\xbb", 1, b"B", OK, 1, 10)
# a code that spans a word boundary: 31 x '0', then '1' | '0' (treePos and next carry over, :126-130 only refills the word)
case("huf20 8-bit, a code spanning a word boundary", HUF8, T8 + words(A_ * 31 + B_ + C_), 33, b"A" * 31 + b"BC", OK, 33, 14)
# 4-bit: symbol i goes to byte i / 2, shifted by 4 when ((i & 1) == 0) ^ little (:145-146): little = low nibble first
T4 = tree3(0x1, 0x2, 0x3)
case("huf20 4-bit, little nibble order (HUF20 / LZ77)", HUF4, T4 + words(A_ + B_ + C_ + A_), 2, bytes([0x21, 0x13]), OK, 2, 10, aux0=0)
case("huf20 4-bit, big nibble order (Level5)", HUF4, T4 + words(A_ + B_ + C_ + A_), 2, bytes([0x12, 0x31]), OK, 2, 10, aux0=1)
# a leaf value above 0xF: the WHOLE tree byte is ORed in, (byte)(v << 4) or v itself (:146)
TX = tree3(0x1F, 0x02, 0xA7)
SIX = A_ + B_ + C_ + C_ + B_ + A_
case("huf20 4-bit, leaf values above 0xF, little", HUF4, TX + words(SIX), 3, bytes([0x1F | 0x20, 0xA7 | 0x70, 0x02 | 0xF0]), OK, 3, 10, aux0=0)
case("huf20 4-bit, leaf values above 0xF, big", HUF4, TX + words(SIX), 3, bytes([0xF0 | 0x02, 0x70 | 0xA7, 0x20 | 0x1F]), OK, 3, 10, aux0=1)
# statuses: nothing is handed to the destination unless the whole decode succeeded (:103-107) -> dst_len 0
case("huf20 missing word", HUF8, T8 + b"\x00\x00\x00", 1, b"", TRUNC, 0, 9)
case("huf20 second word missing", HUF8, T8 + words(A_ * 32), 33, b"", TRUNC, 0, 10)
case("huf20 no header byte", HUF8, b"", 1, b"", TRUNC, 0, 0)
case("huf20 one header byte", HUF8, b"\x02", 1, b"", TRUNC, 0, 1)
case("huf20 decom_len 0 without header bytes", HUF8, b"", 0, b"", TRUNC, 0, 0)
case("huf20 decom_len 0 with one header byte", HUF4, b"\x02", 0, b"", TRUNC, 0, 1)
case("huf20 decom_len 0 reads header and tree", HUF8, T8 + words(A_), 0, b"", OK, 0, 6)
# source.Read(tree) comes back short: zeros, no error (:101) -- with nothing to decode the stream is fine, otherwise the first word is missing
case("huf20 short tree read, decom_len 0", HUF8, bytes([2, 0x80, 0x41]), 0, b"", OK, 0, 3)
case("huf20 short tree read, then no word", HUF8, bytes([2, 0x80, 0x41]), 1, b"", TRUNC, 0, 3)
# treeSize 0: tree[next - direction] is out of range at the first bit (:136) -> IndexOutOfRangeException, Position behind the word
case("huf20 treeSize 0", HUF8, bytes([0, 0x80]) + words("0") + b"\xcc", 1, b"", TRUNC, 0, 6)
case("huf20 treeSize 0, decom_len 0", HUF4, bytes([0, 0x80]), 0, b"", OK, 0, 2)
# root offset 1 with a one-pair tree: next = 4, index 3 or 2 of 2 bytes
case("huf20 index beyond the tree", HUF8, bytes([1, 0x01, 0x41, 0x42]) + words("1") + b"\xdd\xee\xff\x00", 1, b"", TRUNC, 0, 8)
case("huf20 index beyond the tree after a good symbol", HUF8, bytes([1, 0x80, 0x41, 0x05]) + words("01"), 2, b"", TRUNC, 0, 8)
# a stream that decodes into dst_cap < decom_len; a stream error wins over it
case("huf20 dst_cap below decom_len", HUF8, T8 + words(A_ * 8), 8, b"", CAPACITY, 0, None, cap=4)
case("huf20 stream error wins over dst_cap", HUF8, T8 + b"\x00", 8, b"", TRUNC, 0, 7, cap=4)



# codes longer than a word: a chain of 34 nodes, node j = pair j; nodes 0..32 are 0x80 (offset 0: the right child is the next pair, the left
# child a leaf), node 33 is 0xC0 (two leaves).  Leaf j (j < 33) has the code '1' * j + '0', the last two '1' * 33 + '0' / '1' (34 bits).
def chain34():
    t = bytearray([34, 0x80])
    for j in range(33):
        t += bytes([0x30 + j, 0x80 if j < 32 else 0xC0])                  # pair j: leaf j, node j + 1
    return bytes(t + bytes([0x61, 0x62]))                                # pair 33: the two deepest leaves


TC = chain34()
assert len(TC) == 70
case("huf20 a code longer than a word", HUF8, TC + words("1" * 33 + "0" + "0" + "1" * 33 + "1" + "10"), 4, bytes([0x61, 0x30, 0x62, 0x31]), OK, 4, 70 + 12)
# 62 words of '0' codes are 1984 symbols; the words behind them are never read by the loop of :124-130 although they are there (and hold only
# the front of a 34-bit code): Position stops behind word 62
case("huf20 words behind the last symbol's word are not read (64 words present)", HUF8, TC + words("0" * (62 * 32) + "1" * 32 + "1" + "0" * 31), 1984,
     bytes([0x30]) * 1984, OK, 1984, 70 + 248)
case("huf20 the same with the 34-bit code wanted", HUF8, TC + words("0" * (62 * 32) + "1" * 32 + "1" + "0" * 31), 1985,
     bytes([0x30]) * 1984 + bytes([0x61]), OK, 1985, 70 + 256)

if __name__ == "__main__":
    doc = {"format": "rlh", "generator": "tests/golden/make_kats_rlh.py", "cases": CASES}
    with open(os.path.join(HERE, "rlh_kat.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("%d cases" % len(CASES))
