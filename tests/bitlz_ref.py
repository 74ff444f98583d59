"""Pure-Python restatement of the two bit-stream LZ bodies of the reference's .Extended assembly -- CRILAYLA.DecompressHeaderless
(src/AuroraLib.Compression-Extended/CRI/CRILAYLA.cs:123-188) and ALLZ.DecompressHeaderless (Specialized/ALLZ.cs:90-127, IO/FlagReader.cs) --
under the edge rules of include/auroralz.h.  The CPU oracle has neither body, so this is the yardstick of the alz_bitlz_* tests; it is pinned
itself by the hand-assembled known answers of tests/golden/bitlz_kat.json.  It follows the C# line by line and is not fast.

Also here, TEST-ONLY: stream makers (cri_assemble, AllzWriter / allz_assemble), the inverses of the two readers.

cri_decode(src, cap)                               -> (bytes in MEMORY order, status, dst_len, src_used)
allz_decode(src, decom_len, cap, copy, dist, len)  -> (bytes, status, dst_len, src_used)
src_used None = unspecified (a clipped token).  CRILAYLA's bytes are the top of the span: memory [dst_off + cap - dst_len, dst_off + cap)."""

OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
M = 0xFFFFFFFF
VLE_LEVELS = (2, 3, 5, 8)                   # CRILAYLA.cs:129
VLE_FLAGS = (0x3, 0x7, 0x1F, 0xFF)          # CRILAYLA.cs:130
CRI_MAGIC, CRI_HEADER = b"CRILAYLA", 0x100
ALLZ_DEFAULTS = (0, 10, 1)                  # LzCopyBits, LzDistanceBits, LzLengthBits  ALLZ.cs:34-36


class _End(Exception):
    """the managed read beyond the input (IndexOutOfRange / EndOfStream)"""


def i32(v):
    v &= M
    return v - (1 << 32) if v & 0x80000000 else v


def _copy(out, distance, n):
    """out[q] = out[q - distance], byte by byte, n times (overlap replicates)"""
    while n:
        k = min(n, distance)
        a = len(out) - distance
        out += out[a:a + k]
        n -= k


# ---------------------------------------------------------------------------------------------- CRILAYLA
def cri_decode(src, cap):
    src = bytes(src)
    out = bytearray()                        # in the order produced: out[q] lives at destination[cap - 1 - q]
    st = {"sp": len(src) - 1, "flag": 0, "left": 0}           # sourcePointer, bitBuffer, bitsLeft  :125-128

    def get_bits(count):                     # :165-188
        value = 0
        while count > 0:
            if st["left"] == 0:
                if st["sp"] < 0:
                    raise _End()
                st["flag"] = src[st["sp"]]
                st["sp"] -= 1
                st["left"] = 8
            read = min(st["left"], count)
            value = (value << read) & 0xFFFF
            value |= (st["flag"] >> (st["left"] - read)) & ((1 << read) - 1)
            st["left"] -= read
            count -= read
        return value

    status = OK
    try:
        while st["sp"] >= 0:                 # :132
            if get_bits(1) == 1:
                distance = get_bits(13) + 3
                length, vle = 3, 0
                while True:                  # :140-148
                    value = get_bits(VLE_LEVELS[vle])
                    length += value
                    if value != VLE_FLAGS[vle]:
                        break
                    if vle != 3:
                        vle += 1
                if distance > len(out):      # destination[destinationPointer + distance] lies beyond the span
                    status = BAD
                    break
                room = cap - len(out)
                _copy(out, distance, min(length, room))
                if length > room:
                    status = CAPACITY
                    break
            else:
                b = get_bits(8)
                if len(out) >= cap:
                    status = CAPACITY
                    break
                out.append(b)                # :158
    except _End:
        status = TRUNC
    loaded = len(src) - 1 - st["sp"]
    src_used = None if status == CAPACITY else (loaded if status == BAD else len(src))
    return bytes(reversed(out)), status, len(out), src_used


def cri_file_decode(data, cap=None):
    """CRILAYLA.Decompress (:66-99) under the file rules: (rc name, status, bytes, src_used); rc name in ok / format / unsupported / stream"""
    data = bytes(data)
    if len(data) < 16 or data[:8] != CRI_MAGIC:
        return "format", OK, b"", 0
    size, csize = int.from_bytes(data[8:12], "little"), int.from_bytes(data[12:16], "little")
    full = size + CRI_HEADER
    if full >= 1 << 31:
        return "unsupported", OK, b"", 0
    if 16 + csize > len(data):
        return "stream", TRUNC, b"", len(data)
    if cap is not None and cap < full:
        return "stream", CAPACITY, b"", 0
    hdr = data[16 + csize:16 + csize + CRI_HEADER]
    buf = bytearray(full)
    buf[:len(hdr)] = hdr
    out, status, n, _ = cri_decode(data[16:16 + csize], full)
    buf[full - n:] = out
    used = 16 + csize + len(hdr)
    if status == OK and n < size:
        status = MISMATCH
    if status in (OK, MISMATCH):
        return ("ok" if status == OK else "stream"), status, bytes(buf), used
    return "stream", status, b"", used


def cri_field(value, nbits):
    return [(value >> (nbits - 1 - i)) & 1 for i in range(nbits)]


def cri_token_bits(tok):
    """("lit", byte) | ("match", distance, length) | ("bits", [0 / 1, ...]) for anything else"""
    if tok[0] == "lit":
        return [0] + cri_field(tok[1], 8)
    if tok[0] == "bits":
        return list(tok[1])
    _, distance, length = tok
    assert 3 <= distance <= 8194 and length >= 3
    bits = [1] + cri_field(distance - 3, 13)
    rem, vle = length - 3, 0                 # CompressHeaderless  :228-238
    while rem >= VLE_FLAGS[vle]:
        bits += cri_field(VLE_FLAGS[vle], VLE_LEVELS[vle])
        rem -= VLE_FLAGS[vle]
        if vle != 3:
            vle += 1
    return bits + cri_field(rem, VLE_LEVELS[vle])


def cri_assemble(tokens, pad=0):
    """the body that decodes to `tokens`: the first token's first bit is the top bit of the LAST byte; `pad` fills the final byte"""
    bits = [b for t in tokens for b in cri_token_bits(t)]
    bits += [pad] * (-len(bits) % 8)
    by = bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))
    return bytes(reversed(by))


def cri_expected(tokens):
    """what `tokens` produce, in the order produced (no decoder: the definition of the tokens)"""
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            _copy(out, t[1], t[2])
    return bytes(out)


def cri_file(body, size, header=bytes(CRI_HEADER), csize=None):
    return CRI_MAGIC + size.to_bytes(4, "little") + (len(body) if csize is None else csize).to_bytes(4, "little") + body + header


# ---------------------------------------------------------------------------------------------- ALLZ
def allz_decode(src, decom_len, cap=None, copy=0, dist=10, ln=1):
    src = bytes(src)
    cap = decom_len if cap is None else cap
    lim = min(decom_len, cap)
    clip = CAPACITY if cap < decom_len else MISMATCH
    out = bytearray()
    st = {"p": 0, "flag": 0, "left": 0}

    def readbit():                           # FlagReader.Readbit, Endian.Little  FlagReader.cs:53-65
        if st["left"] == 0:
            if st["p"] >= len(src):
                raise _End()
            st["flag"] = src[st["p"]]
            st["p"] += 1
            st["left"] = 8
        shift = 8 - st["left"]
        st["left"] -= 1
        return (st["flag"] >> shift) & 1

    def read_al_flag(start):                 # ALLZ.cs:118-126, in C# int arithmetic
        bits = start
        while readbit():
            bits = i32(bits + 1)
        result = 0
        i = 0
        while i < bits:                      # ReadInt  FlagReader.cs:80-86
            if readbit():
                result |= 1 << (i & 31)
            i += 1
        result = (result + ((((1 << ((bits - start) & 31)) - 1) & M) << (start & 31))) & M
        return i32(result)

    status = OK
    try:
        while len(out) < decom_len:          # :95
            if not readbit():
                run = i32(read_al_flag(ln) + 1)
                if run < 0:
                    status = BAD
                    break
                room = lim - len(out)
                want, have = min(run, room), len(src) - st["p"]
                if have < want:
                    out += src[st["p"]:]
                    st["p"] = len(src)
                    raise _End()
                out += src[st["p"]:st["p"] + want]
                if run > room:
                    status = clip
                    break
                st["p"] += run
            if len(out) < decom_len:         # :104
                distance = i32(read_al_flag(dist) + 1)
                length = i32(read_al_flag(copy) + 3)
                if length <= 0:
                    continue
                if distance <= 0 or distance > len(out):
                    status = BAD
                    break
                room = lim - len(out)
                _copy(out, distance, min(length, room))
                if length > room:
                    status = clip
                    break
    except _End:
        status = TRUNC
    src_used = None if status in (CAPACITY, MISMATCH) else (len(src) if status == TRUNC else st["p"])
    return bytes(out), status, len(out), src_used


class AllzWriter:
    """FlagWriter(destination, Endian.Little) with the placement the lazy reader needs: a flag byte is RESERVED in the stream at the moment the
    first bit of a new group of eight is written; raw bytes go to the current end."""

    def __init__(self):
        self.out = bytearray()
        self.at = None                       # index of the flag byte being filled
        self.n = 0                           # bits in it

    def bit(self, b):
        if self.at is None or self.n == 8:
            self.at, self.n = len(self.out), 0
            self.out.append(0)
        self.out[self.at] |= (b & 1) << self.n
        self.n += 1

    def raw(self, data):
        self.out += bytes(data)

    def rawflag(self, ones, value, nbits):
        """`ones` 1-bits, a 0-bit, then nbits bits of value, least significant first: any ReadALFlag field"""
        for _ in range(ones):
            self.bit(1)
        self.bit(0)
        for i in range(nbits):
            self.bit((value >> i) & 1)

    def alflag(self, start, value):          # WriteALFlag  ALLZ.cs:160-173
        mask, bits = 0, start
        while mask + ((1 << bits) - 1) < value:
            bits += 1
            mask = ((1 << (bits - start)) - 1) << start
        self.rawflag(bits - start, value - mask, bits)

    def bytes(self):
        return bytes(self.out)


def allz_assemble(tokens, copy=0, dist=10, ln=1):
    """("run", bytes) | ("match", distance, length).  A match follows every run unless the run is the last token; a match that follows no run
    is introduced by a 1-bit."""
    w = AllzWriter()
    after_run = False
    for k, t in enumerate(tokens):
        if t[0] == "run":
            assert not after_run and len(t[1]) >= 1, "a match follows every run"
            w.bit(0)
            w.alflag(ln, len(t[1]) - 1)
            w.raw(t[1])
            after_run = True
        else:
            if not after_run:
                w.bit(1)
            w.alflag(dist, t[1] - 1)
            w.alflag(copy, t[2] - 3)
            after_run = False
    return w.bytes()


def allz_expected(tokens):
    out = bytearray()
    for t in tokens:
        if t[0] == "run":
            out += t[1]
        else:
            _copy(out, t[1], t[2])
    return bytes(out)


def allz_file(body, size, copy=0, dist=10, ln=1):
    return b"ALLZ" + bytes([0, copy, dist, ln]) + size.to_bytes(4, "little") + body
