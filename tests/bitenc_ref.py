"""Pure-Python restatement of the two CompressHeaderless bodies and the two Compress methods that alz_bitenc_* writes on the GPU:
CRILAYLA (src/AuroraLib.Compression-Extended/CRI/CRILAYLA.cs:102-121,190-279) and ALLZ (Specialized/ALLZ.cs:78-88,129-174), over the finder of
tests/chain_finder_ref.py.  TEST-ONLY; line by line after the C#, not fast.  Sibling of tests/bitlz_ref.py (the two readers).

cri_compress_headerless(data, quality, strategy=0)                   -> the body, in memory order
allz_compress_headerless(data, quality, copy, dist, ln, strategy=0)  -> the body
cri_compress(data, quality) / allz_compress(data, quality, copy, dist, ln) -> the file"""
import chain_finder_ref as CF
from bitlz_ref import ALLZ_DEFAULTS, CRI_HEADER, CRI_MAGIC, VLE_FLAGS, VLE_LEVELS

CRI_LZ = CF.LzProperties(0x2000, 0xFFFF, 3, 0, 3)                           # CRILAYLA.cs:21
ALLZ_LZ = [CF.LzProperties(0x1000, 0x40000, 3), CF.LzProperties(0x4000, 0x40000, 4), CF.LzProperties(0x8000, 0x40000, 5),
           CF.LzProperties(0x20000, 0x40000, 6), CF.LzProperties(0x80000, 0x40000, 8)]                                      # ALLZ.cs:25-32


def cri_emit(data, match_list):
    """CompressHeaderless :208-246 for a given match list over `data` (ALREADY reversed): SetBits fills the array from its last byte downwards"""
    dest = bytearray(len(data) + len(data) // 8 + 16)                       # (a large enough array: nine bits per literal)
    st = {"dst": len(dest) - 1, "buf": 0, "left": 8}

    def set_bits(value, count):          # :260-279
        while count > 0:
            if st["left"] == 0:
                dest[st["dst"]] = st["buf"]
                st["dst"] -= 1
                st["buf"], st["left"] = 0, 8
            write = min(st["left"], count)
            shift = count - write
            bits = (value >> shift) & ((1 << write) - 1)
            st["buf"] |= (bits << (st["left"] - write)) & 0xFF
            st["left"] -= write
            count -= write

    sp = 0
    for offset, distance, length in match_list:
        for _ in range(offset - sp):
            set_bits(0, 1)
            set_bits(data[sp], 8)
            sp += 1
        if length == 0:
            break
        set_bits(1, 1)
        set_bits((distance - 3) & 0xFFFF, 13)
        vle, rem = 0, length - 3
        while rem >= VLE_FLAGS[vle]:
            set_bits(VLE_FLAGS[vle], VLE_LEVELS[vle])
            rem -= VLE_FLAGS[vle]
            if vle != 3:
                vle += 1
        set_bits(rem, VLE_LEVELS[vle])
        sp += length
    if st["left"] != 8:
        dest[st["dst"]] = st["buf"]
        st["dst"] -= 1
    return bytes(dest[st["dst"] + 1:])


def cri_compress_headerless(data, quality=8, strategy=0):
    rev = bytes(reversed(bytes(data)))                                      # "Our LZMatcher only works in one direction."  :204-206
    return cri_emit(rev, CF.matches(CRI_LZ, rev, quality, 0, strategy))


def cri_compress(data, quality=8, strategy=0):
    """Compress :102-121, with the array the body is written into as large as it needs (the managed one is rented at length + 10 %)"""
    data = bytes(data)
    if len(data) < CRI_HEADER:
        raise ValueError("Source must be at least 256 bytes long.")
    body = cri_compress_headerless(data[CRI_HEADER:], quality, strategy)
    return CRI_MAGIC + (len(data) - CRI_HEADER).to_bytes(4, "little") + len(body).to_bytes(4, "little") + body + data[:CRI_HEADER]


def allz_emit(data, match_list, copy=ALLZ_DEFAULTS[0], dist=ALLZ_DEFAULTS[1], ln=ALLZ_DEFAULTS[2], phases=None):
    """CompressHeaderless :135-158 for a given match list.  phases: a list that receives, per run, the bits of the open flag byte at the moment
    the run is handed over (0: FlushIfNecessary lets it out at once)"""
    flag = CF.FlagWriter(False)          # Endian.Little

    def write_al_flag(start, value):     # :160-173
        mask, bits = 0, start
        while mask + ((1 << bits) - 1) < value:
            bits += 1
            mask = ((1 << (bits - start)) - 1) << start
            flag.write_bit(1)
        flag.write_bit(0)
        flag.write_int(value - mask, bits)

    sp = 0
    for offset, distance, length in match_list:
        plain = offset - sp
        if plain > 0:
            flag.write_bit(0)
            write_al_flag(ln, plain - 1)
            flag.buffer += data[sp:sp + plain]
            if phases is not None:
                phases.append((8 - flag.left) % 8)
            sp += plain
            flag.flush_if_necessary()
        else:
            flag.write_bit(1)
        if sp == len(data):
            break
        write_al_flag(dist, distance - 1)
        write_al_flag(copy, length - 3)
        sp += length
    flag.flush()                         # Dispose
    return bytes(flag.out)


def allz_compress_headerless(data, quality=8, copy=ALLZ_DEFAULTS[0], dist=ALLZ_DEFAULTS[1], ln=ALLZ_DEFAULTS[2], strategy=0):
    data = bytes(data)
    return allz_emit(data, CF.matches(ALLZ_LZ, data, quality, 0, strategy), copy, dist, ln)


def allz_compress(data, quality=8, copy=ALLZ_DEFAULTS[0], dist=ALLZ_DEFAULTS[1], ln=ALLZ_DEFAULTS[2], strategy=0):
    """Compress :78-88"""
    data = bytes(data)
    return b"ALLZ" + bytes([0, copy, dist, ln]) + len(data).to_bytes(4, "little") + allz_compress_headerless(data, quality, copy, dist, ln, strategy)
