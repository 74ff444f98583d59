#!/usr/bin/env python3
"""make_aplib_kats.py -- hand-assembled known answers for the aPLib body (alz_aplib_*).

This script calls NO decoder, not the library and not tests/aplib_ref.py: every stream is written down bit by bit next to the C# statement that
reads it (the reference's src/AuroraLib.Compression/Formats/Common/aPLib.cs), and the expected output, status, dst_len and src_used are written
down by hand from those statements.  tests/test_aplib_cpu.py holds tests/aplib_ref.py against them and re-runs this script so the file cannot
drift; tests/test_gpu_aplib.py holds both kernel families against them.

Output: tests/golden/aplib_kat.json (committed).  src_used null = unspecified (OUTPUT_CAPACITY, include/auroralz.h).  A case whose output is
too long to commit carries `out_sha256` and `out_head` / `out_tail` (64 bytes each) instead of `out`; its stream is built here by the bit writer
below (the inverse of the lazy FlagReader), token by token, and its output by the formula next to it.

How the bits are read (aPLib.cs:105-181):
  FlagReader(source, Endian.Big): a flag BYTE is fetched at the current input position when a bit is needed and none is left, its bits are
  consumed MSB first (IO/FlagReader.cs:53-65).  Data bytes (ReadUInt8) are taken from the current position too, so both interleave.
  :113      the first byte is written as it is
  :116-118  prefix: up to three 1-bits          0 = literal | 10 = match / repeat | 110 = short match / end | 111 = one byte
  :297-307  ReadGamma: value = 1; do { value = value << 1 | bit } while (bit)   -- value bit, "more" bit, value bit, "more" bit, ...
  :288-295  LengthDelta(d): d < 0x80 or d >= 0x7D00 -> 2; d >= 0x500 -> 1; else 0
"""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
CASES = []


def case(name, src, cap, out, status, dst_len, src_used):
    out, src = bytes(out), bytes(src)
    assert len(out) == dst_len
    c = dict(name=name, src=src.hex(), cap=cap, status=status, dst_len=dst_len, src_used=src_used)
    if len(out) <= 4096:
        c["out"] = out.hex()
    else:
        c["out_sha256"] = hashlib.sha256(out).hexdigest()
        c["out_head"], c["out_tail"] = out[:64].hex(), out[-64:].hex()
    CASES.append(c)


# ------------------------------------------------------------------------------------------------ every token kind, by hand
# offset  byte  meaning
#  0      41    :113  first byte 'A'                                                                 out "A"
#  1      72    flag byte F1 = 0111 0010, fetched for the next bit
#                 bit 0          :118 prefix 0 -> :122 literal
#  2      42          ReadUInt8 = 'B'                                                                out "AB"        lwm = false
#                 bits 1 1 1     prefix 3 -> :167
#                 bits 0 0 1 0   ReadInt(4) = 2 -> BackCopy(2, 1): 'A'                               out "ABA"       lwm = false
#  3      c8    flag byte F2 = 1100 1000
#                 bits 1 1 0     prefix 2 -> :151
#  4      07          ReadUInt8 = 7: length = 2 + (7 & 1) = 3, offset = 7 >> 1 = 3 -> BackCopy(3, 3)  out "ABAABA"    lastOffset = 3, lwm = true
#                 bit 0          literal
#  5      43          'C'                                                                            out "ABAABAC"   lwm = false
#                 bits 1 0       prefix 1 -> :126
#                 bits 0 0       ReadGamma: value bit 0, more 0 -> 0b10 = 2; !lwm && 2 == 2 -> repeat, offset = lastOffset = 3
#  6      68    flag byte F3 = 0110 1000
#                 bits 0 1 1 0   ReadGamma: 0 more, 1 last -> 0b101 = 5 -> BackCopy(3, 5): "BACBA"   out "ABAABACBACBA"          lwm = true
#                 bits 1 0       prefix 1
#                 bits 0 0       ReadGamma = 2; lwm -> offset = 2 - 2 = 0
#  7      07          offset = 0 << 8 | 7 = 7
#  8      e8    flag byte F4 = 1110 1000
#                 bits 1 1 1 0   ReadGamma: 1 more, 1 last -> 0b111 = 7; + LengthDelta(7) = 2 -> 9 -> BackCopy(7, 9): "ACBACBA" + "AC"
#                                                                                                    out "ABAABACBACBAACBACBAAC" lastOffset = 7, lwm = true
#                 bits 1 0       prefix 1
#                 bits 0 0       ReadGamma = 2; lwm -> offset = 0
#  9      90          offset = 0x90 = 144
# 10      4e    flag byte F5 = 0100 1110
#                 bits 0 1 0 0   ReadGamma: 0 more, 0 last -> 0b100 = 4; + LengthDelta(144) = 0 -> BackCopy(144, 4): 21 bytes exist, all four sources
#                                lie in front of the stream start -> 00 00 00 00 (E2)                 25 bytes        lastOffset = 144, lwm = true
#                 bits 1 1 1     prefix 3
#                 bit  0         ReadInt(4): first bit
# 11      18    flag byte F6 = 0001 1000
#                 bits 0 0 0     ... = 0 -> WriteByte(0)                                              26 bytes        lwm = false
#                 bits 1 1 0     prefix 2
# 12      00          ReadUInt8 = 0: offset 0 -> return (end)                                         src_used = 13
ALL = bytes.fromhex("41 72 42 c8 07 43 68 07 e8 90 4e 18 00")
ALL_OUT = b"ABAABACBACBAACBACBAAC" + bytes(5)
case("every token kind", ALL, 64, ALL_OUT, OK, 26, 13)
case("every token kind, dst_cap exact", ALL, 26, ALL_OUT, OK, 26, 13)
# the match (7, 9) starts at 12 bytes: with dst_cap 15 it is clipped to 3 bytes (E5)
case("every token kind, dst_cap inside a match", ALL, 15, ALL_OUT[:15], CAPACITY, 15, None)
# ... with dst_cap 2 the one-byte token of F1 does not fit
case("every token kind, dst_cap at a one-byte token", ALL, 2, ALL_OUT[:2], CAPACITY, 2, None)
case("dst_cap 0: the first byte does not fit", ALL, 0, b"", CAPACITY, 0, None)
# bytes behind the end marker are not read
case("bytes behind the end marker", ALL + b"\xff\xff", 64, ALL_OUT, OK, 26, 13)
# the input ends where the low byte of the match (144, 4) is wanted (offset 9): 21 bytes are out
case("input ends at a distance byte", ALL[:9], 64, ALL_OUT[:21], TRUNC, 21, 9)
# ... where flag byte F5 is wanted, inside the length gamma
case("input ends inside a length gamma", ALL[:10], 64, ALL_OUT[:21], TRUNC, 21, 10)
# ... where the end marker's byte is wanted
case("input ends at the end marker's byte", ALL[:12], 64, ALL_OUT, TRUNC, 26, 12)
case("empty input", b"", 64, b"", TRUNC, 0, 0)
# :113 writes the byte, then :117 wants a flag byte
case("one byte", b"\x41", 64, b"A", TRUNC, 1, 1)
#  0  41   first byte
#  1  c0   F1 = 1100 0000: bits 1 1 0 prefix 2
#  2  00   offset 0 -> end
case("first byte and end marker", bytes.fromhex("41 c0 00"), 64, b"A", OK, 1, 3)
#  0  41   first byte
#  1  83   F1 = 1000 0011: bits 1 0 prefix 1; bits 0 0 ReadGamma = 2, !lwm -> repeat with lastOffset = 0; bits 0 0 ReadGamma = 2
#          BackCopy(0, 2): distance 0 = the window size 0x200000 (E1), in front of the stream start (E2) -> 00 00;   lwm = true
#          bits 1 1 of the prefix 1 1 0 ...
#  2  00   F2 = 0000 0000: bit 0
#  3  00   offset 0 -> end
case("repeat as the first token: distance 0", bytes.fromhex("41 83 00 00"), 64, b"A\0\0", OK, 3, 4)

# ------------------------------------------------------------------------------------------------ gamma wrap (the int of ReadGamma overflows)
#  0  01   first byte
#  flag bits: 1 0                          prefix 1
#             gamma (1 << 33) | 5 = 0b1 000...000 101 (34 bits): 33 value bits below the leading one -- thirty zeros, then 1 0 1 --,
#               each followed by "more" = 1 except the last: 66 bits
#               the int keeps the low 32 bits: 5;  !lwm: 5 != 2 -> offset = 5 - 3 = 2
#  data byte  10                           offset = 2 << 8 | 0x10 = 0x210 = 528
#             gamma 4: bits 0 1 0 0        + LengthDelta(528) = 0 -> BackCopy(528, 4): one byte exists -> 00 00 00 00 (E2)
#             1 1 0 + data byte 00         end
class Bits:
    """flag bits MSB first into a byte reserved when its first bit is written (what the lazy reader undoes); data bytes go to the current end"""

    def __init__(self, first):
        self.o, self.fi, self.left = bytearray([first]), -1, 0

    def bit(self, *bs):
        for b in bs:
            if self.left == 0:
                self.fi, self.left = len(self.o), 8
                self.o.append(0)
            self.left -= 1
            self.o[self.fi] |= b << self.left
        return self

    def byte(self, b):
        self.o.append(b)
        return self

    def gamma(self, v):                    # value bits below the leading one, each followed by more (1) / last (0)
        for i in range(v.bit_length() - 2, -1, -1):
            self.bit((v >> i) & 1, 1 if i else 0)
        return self


w = Bits(0x01).bit(1, 0).gamma((1 << 33) | 5).byte(0x10).gamma(4).bit(1, 1, 0).byte(0)
# 2 + 66 + 4 + 3 = 75 flag bits = 10 flag bytes, + first byte + low byte + end byte
assert len(w.o) == 13
case("gamma wraps at 32 bits", w.o, 64, bytes([1, 0, 0, 0, 0]), OK, 5, 13)

# ------------------------------------------------------------------------------------------------ the 2 MiB window
# 64 fixed bytes (the first byte + 63 literals: bit 0 + the byte), then
#   match(64, 2^21 + 36): prefix 1 0; !lwm -> gamma (64 >> 8) + 3 = 3; low byte 0x40; gamma 2^21 + 36 - LengthDelta(64) = 2^21 + 34
#                         the 64 bytes repeat: byte i of the output is START[i % 64] for i < 64 + 2^21 + 36 = 2 097 252
#   lit 0xEE              byte 2 097 252
#   match(2^21, 8):       prefix 1 0; !lwm -> gamma (2^21 >> 8) + 3 = 8195; low byte 0; gamma 8 - LengthDelta(2^21) = 6
#                         distance exactly the window: legal.  Sources 2 097 253 - 2^21 = 101 .. 108 = START[37 .. 44]
#   end                   2 097 261 bytes
START = bytes((37 * i * i + 11 * i + 5) & 0xFF for i in range(64))
FAR_LEN = (1 << 21) + 36


def far_stream(dist):
    w = Bits(START[0])
    for b in START[1:]:
        w.bit(0).byte(b)
    w.bit(1, 0).gamma(3).byte(0x40).gamma(FAR_LEN - 2)
    w.bit(0).byte(0xEE)
    w.bit(1, 0).gamma((dist >> 8) + 3).byte(dist & 0xFF).gamma(8 - 2)
    w.bit(1, 1, 0).byte(0)
    return bytes(w.o)


PERIODIC = (START * ((64 + FAR_LEN) // 64 + 1))[:64 + FAR_LEN]
far_ok = far_stream(1 << 21)
assert len(far_ok) == 87
case("distance = the window (2 MiB)", far_ok, (1 << 21) + 200, PERIODIC + b"\xee" + START[37:45], OK, 2097261, 87)
# one more: offset = 0x2000 << 8 | 1 > 0x200000 -> refused (E3) once the length gamma behind it is read: its last bit sits in the flag byte at
# offset 84 (the stream's last flag byte), so src_used = 85; the end marker's data byte at 86 is never reached
far_bad = far_stream((1 << 21) + 1)
assert len(far_bad) == 87
case("distance = the window + 1", far_bad, (1 << 21) + 200, PERIODIC + b"\xee", BAD, 2097253, 85)

if __name__ == "__main__":
    with open(os.path.join(HERE, "aplib_kat.json"), "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")
    print("wrote %d cases" % len(CASES))
