"""Pure-Python side of the wrapped-file tests (alz_wfile_*): the SSZL keystream restated next to the C# line numbers, and builders of files of all
eight kinds over the standard library's zlib / gzip, each returning the file and the field list a walk must report.  RLHudson's body is
tests/rlhudson_ref.py.  Paths relative to the reference's src/AuroraLib.Compression-Extended."""
import gzip
import random
import struct
import zlib

import rlhudson_ref as RH

ASURAZLB, ZLB, MDF0, RAREZIP, HWGZ, SSZL, ZLWF, RLHUDSON = range(8)
B_ZLIB, B_GZIP, B_DEFLATE, B_WFLZ, B_WFLZ_BE, B_RLHUDSON, B_PLAIN = range(7)
OK, E_INVALID, E_FORMAT, E_STREAM, E_CHECKSUM = 0, -1, -6, -7, -8
COMPRESSED, USE_GZIP, ENCRYPTED = 0x1, 0x2, 0x80000000
M31, M32 = 0x7FFFFFFF, 0xFFFFFFFF


def sszl_keystream(nwords, seed=0x40C360F3):
    """MersenneTwister of Specialized/SSZL.cs:200-282"""
    buf = [0] * 624
    buf[0] = seed & M31                                            # :223
    for i in range(623):                                           # :226-233
        cur = buf[i]
        tmp = cur ^ (cur >> 30)
        mul = (0x13F8769B * tmp) & M32
        buf[i + 1] = ((i + 1) - mul) & M32 & M31
    out, index = [], 624
    for _ in range(nwords):                                        # Next  :239-262
        if index == 624:
            index = 0
        a, b, c = buf[index], buf[(index + 1) % 624], buf[(index + 397) % 624]
        part = (a ^ ((a ^ b) & M31)) >> 1                          # Twist  :264-268
        v = (part ^ c ^ ((0x1908B0DF * (b & 1)) & M32)) & M31
        buf[index] = v
        index += 1
        t1 = (v >> 11) ^ v                                         # Temper  :270-282
        t3 = (((t1 & 0xFF3A58AD) << 7) & M32) ^ t1
        t5 = (((t3 & 0xFFFFDF8C) << 15) & M32) ^ t3
        s = t5 - (1 << 32) if t5 & 0x80000000 else t5              # (int)t5
        out.append((s ^ (s >> 18)) & M31)                          # the arithmetic shift
    return out


def sszl_xor(data):
    """MTXorTransform  :169-195: whole little-endian words, then 1-3 bytes of one more word"""
    ks = sszl_keystream((len(data) + 3) // 4)
    return bytes(b ^ ((ks[i >> 2] >> (8 * (i & 3))) & 0xFF) for i, b in enumerate(data))


def fields(parts, stated, flags=0):
    return dict(parts=[tuple(p) for p in parts], stated=stated, flags=flags)


def asurazlb(data, csize_delta=0, stated_delta=0, z=None):
    z = zlib.compress(data, 6) if z is None else z
    f = b"AsuraZlb" + struct.pack("<I", 1) + struct.pack(">II", len(z) + csize_delta, len(data) + stated_delta) + z
    return f, fields([(20, min(len(z) + csize_delta, len(z)), B_ZLIB, 0)], len(data) + stated_delta)


def zlb(data, csize_delta=-4, stated_delta=0, z=None):
    """csize_delta -4: what the reference's own writer stores (Length - 0x14 behind a 16-byte header)"""
    z = zlib.compress(data, 6) if z is None else z
    f = b"ZLB\0" + struct.pack(">III", 1, len(data) + stated_delta, len(z) + csize_delta) + z
    return f, fields([(16, min(len(z) + csize_delta, len(z)), B_ZLIB, 0)], len(data) + stated_delta)


def mdf0(data, stated_delta=0):
    z = zlib.compress(data, 6)
    return b"mdf\0" + struct.pack("<I", len(data) + stated_delta) + z, fields([(8, len(z), B_ZLIB, 0)], len(data) + stated_delta)


def rarezip(data, stated_delta=0):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = c.compress(data) + c.flush()
    return b"\x11\x72" + struct.pack(">I", len(data) + stated_delta) + z, fields([(6, len(z), B_DEFLATE, 0)], len(data) + stated_delta)


def hwgz(data, chunk, header_big=True, order_big=True):
    """header_big: the order of the three header words (the reader detects it); order_big: the order of the chunk size words (FormatByteOrder)"""
    count = (len(data) + chunk - 1) // chunk
    f = bytearray(struct.pack(">III" if header_big else "<III", chunk, count, len(data)) + bytes(4 * count))
    f += bytes(-len(f) % 128)
    parts = []
    for i in range(count):
        z = zlib.compress(data[i * chunk:(i + 1) * chunk], 6)
        struct.pack_into(">I" if header_big else "<I", f, 12 + 4 * i, len(z) + 4)
        f += struct.pack(">I" if order_big else "<I", len(z))
        parts.append((len(f), len(z), B_ZLIB, 0))
        f += z
        f += bytes(-len(f) % 128)
    return bytes(f), fields(parts, len(data))


def sszl(data, options, use_gzip=False):
    if options & COMPRESSED:
        payload = gzip.compress(data, 6, mtime=0) if use_gzip else zlib.compress(data, 6)
        body = B_GZIP if use_gzip else B_ZLIB
    else:
        payload, body = data, B_PLAIN
    stored = sszl_xor(payload) if options & ENCRYPTED else payload
    f = b"SSZL" + struct.pack("<IIII", 0x20101109, len(data), options, 0) + stored
    return f, fields([(20, len(payload), body, 0)], len(data), options)


def wflz_file(data, big):
    """TEST-ONLY: a WFLZ file whose body holds literals only (blocks 0 / 0 / n + n bytes, block 0 / 0 / 0 ends: WayForward/WFLZ.cs:136-158)"""
    body = b"".join(bytes([0, 0, 0, len(data[k:k + 255])]) + data[k:k + 255] for k in range(0, len(data), 255)) + bytes(4)
    return b"WFLZ" + struct.pack(">II" if big else "<II", len(body), len(data)) + body


def zlwf(data, block, big=True):
    o = ">" if big else "<"
    count = (len(data) + block - 1) // block
    f = bytearray(b"ZLWF" + bytes(4) + struct.pack(o + "II", len(data), count) + bytes(4 * count))
    parts = []
    for i in range(count):
        f += bytes(-len(f) % 16)
        struct.pack_into(o + "I", f, 16 + 4 * i, len(f))
        w = wflz_file(data[i * block:(i + 1) * block], big)
        parts.append((len(f) + 12, len(w) - 12, B_WFLZ_BE if big else B_WFLZ, len(data[i * block:(i + 1) * block])))
        f += w
    f += bytes(-len(f) % 16)
    struct.pack_into(o + "I", f, 4, len(f) - 16)
    return bytes(f), fields(parts, len(data))


def rlhudson(data, stated_delta=0):
    body = RH.rlhudson_encode(data)
    return struct.pack(">II", len(data) + stated_delta, 5) + body, fields([(8, len(body), B_RLHUDSON, len(data) + stated_delta)], len(data) + stated_delta)


def sample(n, seed):
    """compressible bytes without the RLHudson encoder's over-long literal runs"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.randrange(256)]) * rng.choice([1, 2, 3, 5, 40]) + b"abcabcabd"[:rng.randrange(1, 9)]
    out = bytes(out[:n])
    return out if not RH.rlhudson_has_defect(out) else sample(n, seed + 1000)


def corpus():
    """(name, kind, big, file, fields, data, expect) -- expect: (rc, status) of alz_wfile_decompress into stated + 64; status 0 OK, 1 truncated,
    2 size mismatch.  Clean files of every kind and shape, then the decided edge rules."""
    d = sample(3000, 1)
    out = []

    def add(name, kind, big, built, data, expect=(OK, 0)):
        out.append((name, kind, big, built[0], built[1], data, expect))
    add("asurazlb", ASURAZLB, 0, asurazlb(d), d)
    add("zlb as the reference writes it (csize four short)", ZLB, 0, zlb(d), d)
    add("zlb, whole csize", ZLB, 0, zlb(d, 0), d)
    add("mdf0", MDF0, 0, mdf0(d), d)
    add("rarezip", RAREZIP, 0, rarezip(d), d)
    add("rlhudson", RLHUDSON, 0, rlhudson(d), d)
    for nchunk, size in ((1, 700), (2, 2048), (5, 4500)):                 # 5 chunks: a partial last one
        dd = sample(size, 10 + nchunk)
        for hb in (True, False):
            for ob in (True, False):
                add("hwgz %d chunks, header %s, order %s" % (nchunk, "big" if hb else "little", "big" if ob else "little"), HWGZ, int(ob), hwgz(dd, 1024, hb, ob), dd)
    dd = sample(2048, 12)
    add("hwgz, FormatByteOrder disagrees with the file's size words", HWGZ, 0, (hwgz(dd, 1024, True, True)[0], None), dd, (E_STREAM, 1))
    for nchunk in (1, 3):
        dd = sample(900 * nchunk, 20 + nchunk)
        for big in (True, False):
            add("zlwf %d chunks %s" % (nchunk, "big" if big else "little"), ZLWF, int(big), zlwf(dd, 900, big), dd)
    for opts, gz in ((0, False), (COMPRESSED, False), (ENCRYPTED, False), (COMPRESSED | ENCRYPTED, False), (COMPRESSED | ENCRYPTED, True), (COMPRESSED, True)):
        got = {}                                                           # payload lengths 0..3 mod 4 over the four Options combinations + gzip
        for extra in range(64):
            dd = sample(500 + extra, 30 + extra)
            built = sszl(dd, opts, gz)
            k = built[1]["parts"][0][1] % 4
            if k not in got:
                got[k] = True
                add("sszl options %#x%s, payload = %d mod 4" % (opts, " gzip" if gz else "", k), SSZL, 0, built, dd)
        assert len(got) == 4
    # the decided rules
    z = zlib.compress(d, 6)
    bad = z[:-1] + bytes([z[-1] ^ 1])
    add("asurazlb, flipped Adler-32", ASURAZLB, 0, asurazlb(d, z=bad), d, (E_CHECKSUM, 0))
    add("asurazlb, csize four short (trailer outside the bound: unverified)", ASURAZLB, 0, asurazlb(d, -4), d)
    add("asurazlb, csize four short and a flipped Adler-32 nobody looks at", ASURAZLB, 0, asurazlb(d, -4, z=bad), d)
    add("asurazlb, csize beyond the file", ASURAZLB, 0, asurazlb(d, 1000), d)
    add("asurazlb, csize cuts the DEFLATE data", ASURAZLB, 0, asurazlb(d, -40), d, (E_STREAM, 1))
    add("mdf0, trailer cut (not a bounded body)", MDF0, 0, (mdf0(d)[0][:-2], None), d, (E_STREAM, 1))
    for kind, name, fn in ((ASURAZLB, "asurazlb", asurazlb), (ZLB, "zlb", zlb), (MDF0, "mdf0", mdf0)):
        add(name + ", stated size one short", kind, 0, fn(d, stated_delta=-1), d, (E_STREAM, 2))
        add(name + ", stated size one long", kind, 0, fn(d, stated_delta=1), d, (E_STREAM, 2))
    add("rarezip, stated size one short", RAREZIP, 0, rarezip(d, -1), d, (E_STREAM, 2))
    add("rarezip, stated size three long: zeros", RAREZIP, 0, rarezip(d, 3), d + bytes(3))
    for big in (True, False):                                              # no chunk at all: the stated size is still checked, alone or in any batch
        add("zlwf of no chunks, stated size 0, %s" % ("big" if big else "little"), ZLWF, int(big), (zlwf(b"", 900, big)[0], None), b"")      # (16 bytes: IsMatch wants more)
        o = ">" if big else "<"
        f = b"ZLWF" + struct.pack(o + "III", 0, 5, 0)
        add("zlwf of no chunks, stated size 5, %s" % ("big" if big else "little"), ZLWF, int(big), (f, None), b"", (E_STREAM, 2))
    zd = sample(2000, 41)
    zf, zfields = zlwf(zd, 700, False)                       # a chunk whose body runs past / ends short of the size its header states
    for delta, what in ((-3, "runs past"), (3, "ends short of")):
        off = zfields["parts"][1][0] - 12
        g = zf[:off + 8] + struct.pack("<I", 700 + delta) + zf[off + 12:]
        add("zlwf, the second chunk's body %s its stated size" % what, ZLWF, 0, (g, None), zd[:1400 + min(delta, 0)], (E_STREAM, 2))   # delivered: chunk 1 and the stated / decoded bytes of chunk 2
    add("rlhudson, stated size one short", RLHUDSON, 0, rlhudson(d, -1), None, None)      # (the last token decides: left to the body's reference)
    add("rlhudson, stated size one long", RLHUDSON, 0, rlhudson(d, 1), d, (E_STREAM, 1))
    return out
