"""Pure-Python restatement of aPLib.DecompressHeaderless (the reference's src/AuroraLib.Compression/Formats/Common/aPLib.cs:105-181) under the edge
rules of include/auroralz.h, and two test-only stream makers.  What the GPU kernels (alz_aplib_*) are held against: the CPU oracle has no aPLib.

decode(src, cap)             -> (out, status, dst_len, src_used | None)     src_used None = unspecified (OUTPUT_CAPACITY)
assemble(first_byte, tokens) -> bytes      a bit writer that reserves a flag byte at the moment the first bit of a new group is written: the inverse
                                           of the lazy FlagReader (IO/FlagReader.cs:53-65)
greedy(data)                 -> bytes      a simple valid-stream maker.  NOT the managed encoder (LzChainMatchFinder): its bytes mean nothing beyond
                                           "a stream that decodes to data and uses all five token kinds"
"""
OK, TRUNC, MISMATCH, CAPACITY, BAD = 0, 1, 2, 3, 4
W = 1 << 21                  # lzProperties[^1] = LzProperties(0x200000, ...): WindowsBits 21  aPLib.cs:35, :111
M = 0xFFFFFFFF


def s32(v):
    v &= M
    return v - (1 << 32) if v & 0x80000000 else v


class _Trunc(Exception):
    pass


def length_delta(d):         # aPLib.cs:288-295
    if d < 0x80 or d >= 0x7D00:
        return 2
    if d >= 0x500:
        return 1
    return 0


def decode(src, cap):
    src = bytes(src)
    n = len(src)
    out = bytearray()
    st = dict(p=0, bits=0, flag=0)

    def byte():              # source.ReadUInt8()
        if st["p"] >= n:
            raise _Trunc
        b = src[st["p"]]
        st["p"] += 1
        return b

    def bit():               # FlagReader.Readbit, Endian.Big: the flag byte is fetched when a bit is needed and none is left
        if st["bits"] == 0:
            st["flag"] = byte()
            st["bits"] = 8
        st["bits"] -= 1
        return (st["flag"] >> st["bits"]) & 1

    def gamma():             # ReadGamma :297-307, an int in an unchecked context
        v = 1
        while True:
            v = ((v << 1) | bit()) & M
            if not bit():
                return s32(v)

    def lit(b):              # LzWindows.WriteByte; E5
        if len(out) >= cap:
            return False
        out.append(b)
        return True

    def copy(d, L):          # LzWindows.BackCopy(distance, length) :72-100; E1, E2, E5
        if L <= 0:           # LzWindows.cs:80
            return True
        if d == 0:
            d = W            # E1
        ok = True
        if len(out) + L > cap:
            L = cap - len(out)
            ok = False
        q = len(out) - d
        if q < 0:            # E2: in front of the stream start
            z = min(L, -q)
            out.extend(bytes(z))
            L -= z
            q += z
        if L:
            pat = bytes(out[q:])                     # d bytes: the copy is periodic in d
            out.extend((pat * (L // len(pat) + 1))[:L])
        return ok

    last, lwm = 0, False
    try:
        if not lit(byte()):                          # :113
            return bytes(out), CAPACITY, len(out), None
        while True:
            pre = 0
            while pre < 3 and bit():                 # :116-118
                pre += 1
            if pre == 0:                             # :122-125
                if not lit(byte()):
                    return bytes(out), CAPACITY, len(out), None
                lwm = False
            elif pre == 1:                           # :126-149
                g = gamma()
                if not lwm and g == 2:
                    d = last
                    L = gamma()
                else:
                    d = s32((((g - (2 if lwm else 3)) & M) << 8) | byte())
                    L = gamma()
                    if d < 0 or d > W:               # E3 (the length gamma was read first)
                        return bytes(out), BAD, len(out), st["p"]
                    L = s32(L + length_delta(d))
                    last = d
                lwm = True
                if not copy(d, L):
                    return bytes(out), CAPACITY, len(out), None
            elif pre == 2:                           # :151-165
                b = byte()
                L = 2 + (b & 1)
                d = b >> 1
                if d == 0:
                    return bytes(out), OK, len(out), st["p"]
                if not copy(d, L):
                    return bytes(out), CAPACITY, len(out), None
                last = d
                lwm = True
            else:                                    # :167-178
                d = 0
                for _ in range(4):
                    d = (d << 1) | bit()
                if d:
                    if not copy(d, 1):
                        return bytes(out), CAPACITY, len(out), None
                elif not lit(0):
                    return bytes(out), CAPACITY, len(out), None
                lwm = False
    except _Trunc:
        return bytes(out), TRUNC, len(out), n


class Writer:
    """flag bits MSB first into a byte that is reserved when its first bit is written; data bytes go behind whatever has been reserved so far"""

    def __init__(self):
        self.o = bytearray()
        self.fi = -1
        self.left = 0

    def bit(self, b):
        if self.left == 0:
            self.fi = len(self.o)
            self.o.append(0)
            self.left = 8
        self.left -= 1
        if b:
            self.o[self.fi] |= 1 << self.left

    def bits(self, *bs):
        for b in bs:
            self.bit(b)

    def byte(self, b):
        self.o.append(b & 0xFF)

    def gamma(self, v):
        """the bits ReadGamma turns into v: below the leading 1, every value bit followed by 1 = "more" / 0 = "last" (v may exceed 32 bits: it wraps)"""
        assert v >= 2
        for i in range(v.bit_length() - 2, -1, -1):
            self.bit((v >> i) & 1)
            self.bit(1 if i > 0 else 0)


def assemble(first, tokens):
    """tokens: ('lit', b)  ('one', off 0..15)  ('short', d 1..127, L 2..3)  ('match', d, L)  ('rep', L)  ('end',)
    and, for streams no encoder writes, ('gmatch', g, low, lg): prefix 10, gamma g, the low byte (unless g reads as a repeat), gamma lg -- raw values.
    Tracks lwm / lastOffset as the decoder does, so the gamma bias (2 or 3) of 'match' is right."""
    w = Writer()
    w.byte(first)
    lwm, last = False, 0
    for t in tokens:
        k = t[0]
        if k == "lit":
            w.bit(0); w.byte(t[1]); lwm = False
        elif k == "one":
            w.bits(1, 1, 1); w.bits(*[(t[1] >> i) & 1 for i in (3, 2, 1, 0)]); lwm = False
        elif k == "short":
            assert 1 <= t[1] <= 127 and t[2] in (2, 3)
            w.bits(1, 1, 0); w.byte((t[1] << 1) | (t[2] - 2)); last = t[1]; lwm = True
        elif k == "end":
            w.bits(1, 1, 0); w.byte(0)
        elif k == "rep":
            assert not lwm, "a repeat can only follow a literal / one-byte token"
            w.bits(1, 0); w.gamma(2); w.gamma(t[1]); lwm = True
        elif k == "match":
            d, L = t[1], t[2]
            hi = (d >> 8) + (2 if lwm else 3)
            assert lwm or hi != 2
            w.bits(1, 0); w.gamma(hi); w.byte(d); w.gamma(L - length_delta(d)); last = d; lwm = True
        elif k == "gmatch":
            g, low, lg = t[1], t[2], t[3]
            w.bits(1, 0); w.gamma(g)
            if not (not lwm and (g & M) == 2):
                w.byte(low)
                last = s32((((g - (2 if lwm else 3)) & M) << 8) | (low & 0xFF))
            w.gamma(lg); lwm = True
        else:
            raise ValueError(k)
    return bytes(w.o)


def greedy_tokens(data):
    """(first byte, tokens) of greedy(data)"""
    data = bytes(data)
    toks = []
    i, n, lwm, last, tab = 1, len(data), False, 0, {}

    def ins(p):
        if p + 3 <= n:
            tab.setdefault(data[p:p + 3], []).append(p)
    ins(0)
    while i < n:
        d, L = 0, 0
        for c in reversed(tab.get(data[i:i + 3], [])[-16:]):
            k = 0
            while i + k < n and data[c + k] == data[i + k]:
                k += 1
            if k > L:
                d, L = i - c, k
        if not lwm and last and last <= i and L < 8:              # a repeat of the last distance, when it gives at least two bytes
            k = 0
            while i + k < n and data[i + k - last] == data[i + k]:
                k += 1
            if k >= 2 and k >= L:
                d, L = last, k
        if L >= 2 and d <= W and (d == last and not lwm or (L <= 3 and d <= 127) or L - length_delta(d) >= 2):
            if not lwm and d == last:
                toks.append(("rep", L))
            elif L <= 3 and d <= 127:
                toks.append(("short", d, L))
            else:
                toks.append(("match", d, L))
            last, lwm = d, True
            for k in range(L):
                ins(i + k)
            i += L
            continue
        b, off = data[i], -1
        if b == 0:
            off = 0
        else:
            for k in range(1, min(16, i + 1)):
                if data[i - k] == b:
                    off = k
                    break
        toks.append(("one", off) if off >= 0 else ("lit", b))
        lwm = False
        ins(i)
        i += 1
    toks.append(("end",))
    return data[0], toks


def greedy(data):
    """A test-only valid-stream maker -- NOT the managed encoder.  Emits all five token kinds; needs at least one byte."""
    first, toks = greedy_tokens(data)
    return assemble(first, toks)
