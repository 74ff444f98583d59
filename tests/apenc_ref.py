"""Pure-Python restatement of aPLib.CompressHeaderless and aPLib.Compress (src/AuroraLib.Compression/Formats/Common/aPLib.cs:183-286, :87-103), the body
and the file alz_apenc_* writes on the GPU, over the finder of tests/chain_finder_ref.py.  TEST-ONLY; line by line after the C#, not fast.  Sibling of
tests/aplib_ref.py (the reader and an independent assembler) and tests/bitenc_ref.py (the other two bit-stream bodies).

compress_headerless(data, quality=8, strategy=0) -> the body
compress(data, quality=8, strategy=0)            -> the "AP32" file
emit(data, match_list, stats=None, trace=None)   -> the body for a given match list [(offset, distance, length), ..., (len(data), 0, 0)]; stats: a dict that
                                                    counts the token kinds written and the visits of the `lengthDelta < 2` branch ("dead"); trace: a list
                                                    that receives (kind, position, bits written before the token, distance, length) per token
bound(n)                                         -> alz_apenc_bound"""
import chain_finder_ref as CF
from aplib_ref import length_delta

INT_MAX = 0x7FFFFFFF
APLIB_LZ = [CF.LzProperties(0x1000, INT_MAX, 3), CF.LzProperties(0x80, 3, 2), CF.LzProperties(0x4000, INT_MAX, 4), CF.LzProperties(0x10000, INT_MAX, 5),
            CF.LzProperties(0x40000, INT_MAX, 6), CF.LzProperties(0x100000, INT_MAX, 7), CF.LzProperties(0x200000, INT_MAX, 8)]          # aPLib.cs:27-36


def write_gamma(flag, value):            # :309-319
    assert value >= 1
    k = value.bit_length()
    for i in range(k - 2, -1, -1):
        flag.write_bit((value >> i) & 1)
        flag.write_bit(1 if i > 0 else 0)


class _Writer(CF.FlagWriter):
    """FlagWriter that also counts the bits written (for the tests' traces)"""

    def __init__(self):
        CF.FlagWriter.__init__(self, True)                                  # Endian.Big
        self.nbits = 0

    def write_bit(self, bit):
        self.nbits += 1
        CF.FlagWriter.write_bit(self, bit)


def _emit(data, next_match, stats=None, trace=None):
    """CompressHeaderless :185-285 with FindNextBestMatch as a callable.  trace: a list that receives, per token, (kind, position, bits written before it,
    distance, length) -- kind one of "one", "lit", "rep", "short", "match" (lwm set), "match_biased" (lwm clear), "end"""
    data = bytes(data)
    note = (lambda *t: trace.append(t)) if trace is not None else (lambda *t: None)
    count = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    src_ptr, last_offset, lwm = 0, 0, False
    flag = _Writer()
    first = data[src_ptr]                # destination.WriteByte(source[srcPtr++]): an empty source throws  :191
    src_ptr += 1
    while True:
        offset_m, distance, length = next_match()
        plain = offset_m - src_ptr
        while plain != 0:
            plain -= 1
            by = data[src_ptr]
            src_ptr += 1
            lwm = False
            offset = -1                  # a single-byte match  :205-219
            if by == 0:
                offset = 0
            else:
                lookback = min(16, src_ptr)
                for i in range(1, lookback):
                    if data[src_ptr - 1 - i] == by:
                        offset = i
                        break
            if offset != -1:
                note("one", src_ptr - 1, flag.nbits, offset, 1)
                flag.write_bit(1)
                flag.write_bit(1)
                flag.write_bit(1)
                for i in range(3, -1, -1):                                  # WriteInt(offset, 4, true): most significant bit first
                    flag.write_bit((offset >> i) & 1)
                count("one")
                continue
            note("lit", src_ptr - 1, flag.nbits, 0, 1)
            flag.buffer.append(by)       # :231-232
            flag.write_bit(0)
            count("lit")
        if length == 0:
            break
        if not lwm and last_offset == distance and length >= 2:             # repeat  :239-245
            note("rep", src_ptr, flag.nbits, distance, length)
            flag.write_bit(1)
            flag.write_bit(0)
            write_gamma(flag, 2)
            write_gamma(flag, length)
            count("rep")
        elif length <= 3 and distance <= 127:                               # short block  :246-252
            note("short", src_ptr, flag.nbits, distance, length)
            flag.write_bit(1)
            flag.write_bit(1)
            flag.buffer.append(((distance << 1) | (length - 2)) & 0xFF)
            flag.write_bit(0)
            count("short")
        else:                                                               # normal block  :253-275
            ld = length - length_delta(distance)
            if ld < 2:                   # :256-259 -- never taken for what the finder returns (tests/test_apenc_cpu.py)
                count("dead")
                continue
            note("match" if lwm else "match_biased", src_ptr, flag.nbits, distance, length)
            flag.write_bit(1)
            flag.write_bit(0)
            high = (distance >> 8) + 2
            if not lwm:
                high += 1                # the pair bias
            write_gamma(flag, high)
            flag.buffer.append(distance & 0xFF)
            flag.flush_if_necessary()
            write_gamma(flag, ld)
            count("match" if lwm else "match_biased")
        last_offset = distance
        lwm = True
        src_ptr += length
    note("end", src_ptr, flag.nbits, 0, 0)
    flag.write_bit(1)                    # the end marker  :282-285
    flag.write_bit(1)
    flag.buffer.append(0)
    flag.write_bit(0)
    flag.flush()                         # Dispose
    return bytes([first]) + bytes(flag.out)


def emit(data, match_list, stats=None, trace=None):
    it = iter(match_list)
    return _emit(data, lambda: next(it), stats, trace)


def compress_headerless(data, quality=8, strategy=0, stats=None, trace=None):
    data = bytes(data)
    f = CF.ChainFinder(APLIB_LZ, quality, 0, strategy)
    return _emit(data, lambda: f.find_next_best_match(data), stats, trace)


def compress(data, quality=8, strategy=0):
    """Compress :87-103"""
    data = bytes(data)
    body = compress_headerless(data, quality, strategy)
    w = lambda v: v.to_bytes(4, "little")
    return b"AP32" + w(24) + w(len(body)) + w(0) + w(len(data)) + w(0) + body


def bound(n):
    return n + 1 + (n + 2 + 7) // 8 if n else 0
