"""Python mirror of the reference's format classes (ICompressionAlgorithm surface) over the C ABI container layer.

Same member names and argument meaning as the managed classes so the parity tests read like the reference's own
(CompressionTest/CompressionAlgorithmTest.cs).  All work happens in libauroralz.so: header code in
csrc/alz_container.cpp, bodies on the GPU.  No CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _abi as A
from ._lib import AlzError, check, load


class DecompressedSizeException(Exception):
    """src/AuroraLib.Compression/Exceptions/DecompressedSizeException.cs"""


class EndOfStreamException(EOFError):
    pass


class InvalidIdentifierException(ValueError):
    pass


class InvalidDataException(ValueError):
    """System.IO.InvalidDataException (LZ4 frame checksum mismatch, LZ4.Frame.cs:27)."""


class CompressionSettings:
    """src/AuroraLib.Compression/CompressionSettings.cs:11-84"""

    def __init__(self, quality=8, max_window_bits=0, strategy=0):
        if not 0 <= quality <= 15:
            raise ValueError("quality")
        self.Quality, self.MaxWindowBits, self.Strategy = quality, max_window_bits, strategy


CompressionSettings.Fastest = CompressionSettings(0)
CompressionSettings.Fast = CompressionSettings(4)
CompressionSettings.Balanced = CompressionSettings(8)
CompressionSettings.High = CompressionSettings(12)
CompressionSettings.Maximum = CompressionSettings(15)

_ctx = None


def _context():
    global _ctx
    if _ctx is None:
        from .batch import Context
        _ctx = Context(0)
    return _ctx


def _raise_for_outcome(rc, status, dst_len):
    """rc / status of a container call as the reference's exception types"""
    if rc == A.E_FORMAT:
        raise InvalidIdentifierException()
    if rc == A.E_CHECKSUM:
        raise InvalidDataException("Checksum mismatch")
    if rc == A.E_STREAM:
        if status == A.ST_INPUT_TRUNCATED:
            raise EndOfStreamException()
        if status == A.ST_OUTPUT_SIZE_MISMATCH:
            raise DecompressedSizeException(dst_len)
        if status == A.ST_OUTPUT_CAPACITY:
            raise BufferError("destination too small")    # NotSupportedException of a fixed-size stream
        raise ValueError("bad token")
    check(rc)


def _alz_settings(settings):
    """the alz_settings* of a call from a CompressionSettings (None: Balanced)"""
    s = settings or CompressionSettings.Balanced
    return C.byref(A.Settings(s.Quality, s.MaxWindowBits, s.Strategy, 0))


def _keeps_src_used(reader):
    """the `used` of _single for a class that keeps the count as last_src_used"""
    return lambda n: setattr(reader, "last_src_used", n)


def _single(fn, head, data, cap, used=None, used_after=False):
    """One file through fn(ctx, *head, src, src_len, dst, cap, &dst_len[, &src_used, &status]) -> the bytes it left.  The destination is untouched
    memory (np.empty: create_string_buffer writes the whole capacity first -- 68 MB of zeros for a 67 MB frame).  used: the call is a read -- fn has
    the last two arguments, its outcome is raised as the reference's exception, and used(src_used) runs before that (used_after: only once the outcome
    has passed).  None: a write, a failure is an AlzError."""
    dst_arr = np.empty(max(cap, 1), dtype=np.uint8)
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = fn(_context().h, *head, data, len(data), dst_arr.ctypes.data_as(C.c_void_p), cap, C.byref(dl), *(() if used is None else (C.byref(su), C.byref(st))))
    if used is None:
        check(rc)
    elif used_after:
        _raise_for_outcome(rc, st.value, dl.value)
        used(su.value)
    else:
        used(su.value)
        _raise_for_outcome(rc, st.value, dl.value)
    return dst_arr[:dl.value].tobytes()


def _file_error(r, i, entry):
    """What the alz_file_result of file i stands for: None (its bytes are good) or an exception instance -- the instance is the result.  entry: the
    batch wrote the files, a failure is the AlzError of that entry point; None: it read them, a failure is what Decompress raises."""
    if entry is not None:
        return AlzError(r.rc, "%s: file %d" % (entry, i)) if r.rc else None
    try:
        _raise_for_outcome(r.rc, r.status, r.dst_len)
    except Exception as e:
        return e
    return None


def _source(files):
    """the sources of a batch back to back in one buffer, one byte of padding behind the last"""
    return np.frombuffer(b"".join(files) + bytes(1), dtype=np.uint8)


def _table(files, caps, kind=0, aux0=0, align=16):
    """The stream table of one batch over `files` as _source lays them out: file i gets caps[i] bytes of destination (None: no row), every
    destination starts where the one before ends, rounded up to `align` bytes (1: back to back; 0: a measure pass, dst_off stays 0).  `kind` is
    what Stream.format of the batch family takes.  -> (table, dst_bytes)"""
    rows, so, do = [], 0, 0
    for f, cap in zip(files, caps):
        if cap is not None:
            rows.append(A.Stream(so, do, len(f), cap, 0, aux0, 0, kind))
            do += (cap + align - 1) // align * align if align else 0
        so += len(f)
    return (A.Stream * len(rows))(*rows), do


def _cut(table, dst, res, entry=None):
    """per row of the table its bytes out of dst -- or the exception instance of _file_error"""
    out = []
    for i, (row, r) in enumerate(zip(table, res)):
        e = _file_error(r, i, entry)
        out.append(e if e is not None else dst[int(row.dst_off):int(row.dst_off) + r.dst_len].tobytes())
    return out


def _batch(files, caps, run, kind=0, aux0=0, align=16, extra=0, entry=None, call_empty=True):
    """Whole files through ONE batch: run(table, src, dst_bytes) -> (dst, results) over _table / _source of them, the destination `extra` bytes longer
    than the slots; call_empty: an empty list is a call with n = 0 (False: no call).  Returns a list with, per file, its bytes or its exception instance."""
    if not files and not call_empty:
        return []
    table, dst_bytes = _table(files, caps, kind, aux0, align)
    dst, res = run(table, _source(files), dst_bytes + extra)
    return _cut(table, dst, res, entry)


def _decompress_many(files, kind, limit, measure_batch, decode_batch, decode_decides=False):
    """The two GPU batches behind every DecompressMany: measure_batch(table, src) gives the sizes up to `limit`, the destination holds exactly
    the measured sizes, decode_batch(table, src, dst_bytes) fills it.  `kind` is what Stream.format of the batch family takes for the class.
    decode_decides: a file whose measure ends in a stream error other than the limit is decoded as well, into the bytes it produces up to
    there, and the decode's outcome is the file's (Decompress decodes first: a wrong content checksum in front of a truncated frame, a
    Snappy chunk the decoder refuses).  Returns a list with, per file, its bytes -- or the exception instance Decompress would have raised."""
    files = [bytes(f) for f in files]
    src = _source(files)
    table, _ = _table(files, [limit] * len(files), kind, align=0)
    measured = measure_batch(table, src) if files else []
    out = [_file_error(r, i, None) for i, r in enumerate(measured)]
    caps = [r.dst_len if e is None or (decode_decides and r.rc == A.E_STREAM and r.status != A.ST_OUTPUT_CAPACITY) else None for r, e in zip(measured, out)]
    good = [i for i, cap in enumerate(caps) if cap is not None]
    if good:
        sub, dst_bytes = _table(files, caps, kind, align=1)
        dst, res = decode_batch(sub, src, dst_bytes)
        for i, result in zip(good, _cut(sub, dst, res)):
            out[i] = result
    return out


class _Format:
    container = None
    provides_size = True
    first_guess_failures = (BufferError,)     # what Decompress without a capacity raises when its first guess was too small

    def __init__(self):
        self.FormatByteOrder = "Big"      # IEndianDependentFormat.FormatByteOrder default (Yaz0.cs:30, PRS.cs:24)
        self.MemoryAlignment = 0          # Yaz0.MemoryAlignment
        self.lz = None
        self.Type = 0                     # LZ77.Type / Level5.Type (0 = class default)
        self.ChunkSize = 0                # LZ77.ChunkSize (0 = 0x1000)
        self.Key = 0                      # LZ00: keystream seed of the next Compress
        self.Name = ""                    # LZ00.Name ("" = "Temp.dat")

    def _opt(self):
        o = A.ContainerOptions()
        o.big_endian = 1 if self.FormatByteOrder == "Big" else 0
        o.memory_alignment = self.MemoryAlignment
        o.variant, o.chunk_size = self.Type, self.ChunkSize
        o.key = self.Key & 0xFFFFFFFF
        nm = self.Name.encode("latin-1")[:32]
        for i, b in enumerate(nm):
            o.name[i] = b
        if self.lz is not None:
            o.lz = self.lz
        return o

    def IsMatch(self, data):
        data = bytes(data)
        return bool(load().alz_container_is_match(self.container, data, len(data)))

    def _capacity_hint(self, data):
        """An upper bound on the decompressed size that the container's framing gives away without decoding (None: none)."""
        return None

    def GetDecompressedSize(self, data):
        if not self.provides_size:
            raise NotImplementedError("%s does not implement IProvidesDecompressedSize" % type(self).__name__)
        data = bytes(data)
        size, o = C.c_uint32(), self._opt()
        rc = load().alz_container_decompressed_size(self.container, C.byref(o), data, len(data), C.byref(size))
        if rc == A.E_FORMAT:
            raise InvalidIdentifierException()
        check(rc)
        return size.value

    def Decompress(self, data, capacity=None):
        """ICompressionDecoder.Decompress: returns the decompressed bytes; raises the reference's exception types.
        Formats without a size field start from a guess (a managed Stream grows by itself); when it does not hold the size is measured."""
        data = bytes(data)
        if capacity is None and not self.provides_size:
            hint = self._capacity_hint(data)
            try:
                return self.Decompress(data, hint if hint is not None else max(len(data) * 8, 1 << 16))
            except self.first_guess_failures:
                pass                                       # (more than the guess: a frame whose blocks decode to more than their nominal size, a long run)
            except MemoryError:
                pass                                       # (a hint the host or the device cannot back: the measured size is what the file needs)
            except AlzError as e:
                if e.code != A.E_NOMEM:
                    raise
            # the first guess did not hold: ONE size query on the GPU, then a decode into exactly that much (at most two decodes, and never a
            # destination larger than the file needs)
            return self.Decompress(data, self.MeasureDecompressedSize(data))
        if capacity is None and getattr(self, "size_either_order", False):
            # Yaz0.Decompress retries with the size field byte-swapped (Yaz0.cs:66-78) into a stream that grows by itself: the
            # capacity is the reading in FormatByteOrder unless that one is absurd, the other reading when it was not enough
            n = self.GetDecompressedSize(data)
            m = int.from_bytes(n.to_bytes(4, "big"), "little")
            first = n if n <= (256 << 20) else m
            try:
                return self.Decompress(data, first + 273)
            except BufferError:
                if max(n, m) <= first or max(n, m) > (1 << 31):
                    raise
                return self.Decompress(data, max(n, m) + 273)
        if capacity is None:
            capacity = self.GetDecompressedSize(data) + 273
        o = self._opt()
        return _single(load().alz_container_decompress, (self.container, C.byref(o)), data, capacity, _keeps_src_used(self), used_after=True)

    def MeasureDecompressedSize(self, data, limit=A.MEASURE_NO_BOUND):
        """The decompressed size of a file of a format WITHOUT a size field (PRS, LZO, FastLZ, LZ4, LZ4Legacy, Snappy), measured on the GPU
        without decoding (alz_container_measure).  Raises what Decompress raises for truncated / bad input, and BufferError when the file decodes
        to more than `limit` bytes (a bound against decompression bombs; the default is the largest size the library counts to)."""
        if self.provides_size:
            raise NotImplementedError("%s states its size: GetDecompressedSize" % type(self).__name__)
        data = bytes(data)
        o = self._opt()
        size, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
        rc = load().alz_container_measure(_context().h, self.container, C.byref(o), data, len(data), limit, C.byref(size), C.byref(su), C.byref(st))
        _raise_for_outcome(rc, st.value, size.value)
        return size.value

    def Compress(self, data, settings=None):
        data = bytes(data)
        o, lib = self._opt(), load()
        return _single(lib.alz_container_compress, (self.container, C.byref(o), _alz_settings(settings)), data, lib.alz_container_compress_bound(self.container, len(data)))


class LZSS(_Format):
    """src/AuroraLib.Compression/Formats/Common/LZSS.cs"""
    container = A.C_LZSS

    def __init__(self, lz=None):
        super().__init__()
        self.lz = lz


class LZ10(_Format):
    container = A.C_LZ10


class LZ11(_Format):
    container = A.C_LZ11


class Yaz0(_Format):
    size_either_order = True
    container = A.C_YAZ0


class Yay0(_Format):
    container = A.C_YAY0


class MIO0(_Format):
    container = A.C_MIO0


class PRS(_Format):
    container, provides_size = A.C_PRS, False
    # PRS.Decompress reads a file that failed again in the other byte order (PRS.cs:42-57), so a destination that was too small surfaces as
    # whatever the OTHER order ends in; the size query that follows has no bound and raises what the file itself deserves
    first_guess_failures = (BufferError, EndOfStreamException, DecompressedSizeException, ValueError)

    def MeasureDecompressedSize(self, data, limit=A.MEASURE_NO_BOUND):
        # PRS.Decompress reads a file that failed again in the other byte order (PRS.cs:42-57), and "the limit was reached" is such a failure: the
        # size is counted without a bound (counting allocates nothing) and held against the limit here
        size = super().MeasureDecompressedSize(data)
        if size > limit:
            raise BufferError("destination too small")
        return size


class LZO(_Format):
    container, provides_size = A.C_LZO, False


# header-only wrappers over the same GPU bodies
class GCLZ(_Format):
    container = A.C_GCLZ


class CXLZ(_Format):
    container = A.C_CXLZ


class LZ_3DS(_Format):
    container = A.C_LZ_3DS


class COMP(_Format):
    container = A.C_COMP


class Yaz1(_Format):
    size_either_order = True
    container = A.C_YAZ1


class AKLZ(_Format):
    container = A.C_AKLZ


class LZ01(_Format):
    container = A.C_LZ01


class LZSega(_Format):
    container = A.C_LZSEGA


class HIG(_Format):
    """src/AuroraLib.Compression-Extended/Specialized/HIG.cs -- High Impact Games WAD LZ; writes version 6 with the default path."""
    container = A.C_HIG


class LZShrek(_Format):
    """src/AuroraLib.Compression-Extended/Activision/LZShrek.cs -- groups of literals + up to eight matches."""
    container = A.C_LZSHREK


class WFLZ(_Format):
    """src/AuroraLib.Compression-Extended/WayForward/WFLZ.cs -- 4-byte blocks + literals; FormatByteOrder defaults to little."""
    container = A.C_WFLZ

    def __init__(self):
        super().__init__()
        self.FormatByteOrder = "Little"           # WFLZ.cs:31


class RefPack(_Format):
    """src/AuroraLib.Compression-Extended/EA/RefPack.cs -- EA's RefPack / QFS; reads header versions 1-3, writes version 2."""
    container = A.C_REFPACK


class LZ02(_Format):
    """src/AuroraLib.Compression-Extended/Camelot/LZ02.cs -- flag-byte LZ that ends at a terminator token."""
    container = A.C_LZ02


class CNS(_Format):
    """src/AuroraLib.Compression-Extended/Specialized/CNS.cs -- byte-oriented runs / matches, 256-byte window."""
    container = A.C_CNS


class CLZ0(_Format):
    """src/AuroraLib.Compression-Extended/Marvelous/CLZ0.cs -- LZSS family, LSB-first flags with 1 = match."""
    container = A.C_CLZ0


class BLZ(_Format):
    """src/AuroraLib.Compression.Nintendo/Nintendo/BLZ.cs -- backwards LZ: code section stored back to front + footer."""
    container = A.C_BLZ


class CNX2(_Format):
    """src/AuroraLib.Compression.Sega/Sega/CNX2.cs -- 2-bit codes (skip / literal / match / literal run), 2 KiB window."""
    container = A.C_CNX2


class FastLZ(_Format):
    """src/AuroraLib.Compression/Formats/Common/FastLZ.cs -- headerless FastLZ stream (levels 1 / 2 decode, level 1 encode)."""
    container = A.C_FASTLZ
    provides_size = False


class LZ00(_Format):
    """src/AuroraLib.Compression.Sega/Sega/LZ00.cs -- LZSS body behind the StreamTransformer keystream.  Compress(data,
    settings, key=None): the managed parameterless overload seeds the keystream with the Unix time (LZ00.cs:64-68)."""
    container = A.C_LZ00

    def Compress(self, data, settings=None, key=None):
        import time
        self.Key = int(time.time()) if key is None else key
        return super().Compress(data, settings)

    def Decompress(self, data, capacity=None):
        out = super().Decompress(data, capacity)
        self.Name = bytes(data[16:48]).split(b"\0")[0].decode("latin-1")     # Name = source.ReadString(32)  LZ00.cs:50
        return out


class Level5LZSS(_Format):
    container = A.C_LEVEL5LZSS


class LZOn(_Format):
    container = A.C_LZON


class _FramedMany:
    """DecompressMany of the classes whose files decode in batches (alz_framed_*): LZ4, LZ4Legacy, Snappy"""

    def DecompressMany(self, files, limit=A.MEASURE_NO_BOUND):
        """Decompress for a whole set of files in two GPU batches: one alz_framed_measure_batch (sizes up to `limit`), a destination of exactly
        the measured sizes, one alz_framed_decode_batch.  Returns a list with, per file, its bytes -- or the exception instance Decompress would
        have raised for it."""
        ctx = _context()
        return _decompress_many(files, self.container, limit, ctx.framed_measure_batch, ctx.framed_decode_batch, decode_decides=True)

    def CompressMany(self, datas, settings=None):
        """Compress for a whole set of inputs in ONE alz_framing_compress_batch: capacities from alz_container_compress_bound, an LZ4 frame's
        block size from ChunkSize.  Returns a list with, per input, the file's bytes -- or the exception instance Compress would have raised."""
        datas = [bytes(d) for d in datas]
        s = settings or CompressionSettings.Balanced
        lib = load()

        def run(table, src, dst_bytes):
            return _context().framing_compress_batch(table, src, dst_bytes, quality=s.Quality, strategy=s.Strategy, max_window_bits=s.MaxWindowBits)
        return _batch(datas, [lib.alz_container_compress_bound(self.container, len(d)) for d in datas], run, self.container, self.ChunkSize, align=1,
                      entry="alz_framing_compress_batch", call_empty=False)


class LZ4(_FramedMany, _Format):
    """src/AuroraLib.Compression/Formats/Common/LZ4.cs + LZ4.Frame.cs: frame (default), legacy and skippable frames.
    BlockSize: 0x10000 / 0x40000 / 0x100000 / 0x400000 (default).  As in the reference, Compress writes a descriptor with
    only the version flag (`Flags &= IsVersion1`, LZ4.Frame.cs:184)."""
    container = A.C_LZ4_FRAME
    provides_size = False
    Block64KB, Block256KB, Block1MB, Block4MB = 0x10000, 0x40000, 0x100000, 0x400000

    def __init__(self, BlockSize=0):
        super().__init__()
        self.ChunkSize = BlockSize

    def _capacity_hint(self, data):
        return _lz4_capacity_hint(data)


def _lz4_capacity_hint(data):
        """blocks x the frame's maximum block size (LZ4.Frame.cs:107-174: FLG, BD, optional content size / dictionary id, header checksum; then u32 sizes; a legacy file:
        blocks of at most 8 MiB, LZ4.cs:96-111) -- a 67 MB frame made the growing loop decode twice, the second time into 256 MB.  None: not a file this walk understands."""
        total, pos, n = 0, 0, len(data)
        if n >= 8 and int.from_bytes(data[:4], "little") == 0x184C2102:
            pos = 4
            while pos + 4 <= n:
                bs = int.from_bytes(data[pos:pos + 4], "little")
                if bs in (0x184D2204, 0x184C2102) or (bs & 0xFFFFFFF0) == 0x184D2A50:
                    return None                            # (another file behind this one: the growing loop's)
                if pos + 4 + bs > n:
                    break
                total += 0x800000; pos += 4 + bs
                if pos < n and data[pos] == 0xFF:
                    break
            return _lz4_clamp_hint(total, n)
        while pos + 7 <= n and int.from_bytes(data[pos:pos + 4], "little") == 0x184D2204:
            flg, bd = data[pos + 4], data[pos + 5]
            bmax = {4: 0x10000, 5: 0x40000, 6: 0x100000, 7: 0x400000}.get((bd >> 4) & 7)
            if bmax is None:
                return None
            pos += 7 + (8 if flg & 8 else 0) + (4 if flg & 1 else 0)
            while pos + 4 <= n:
                bsz = int.from_bytes(data[pos:pos + 4], "little"); pos += 4
                if bsz == 0:
                    break
                total += bmax
                pos += (bsz & 0x7FFFFFFF) + (4 if flg & 16 else 0)
            pos += 4 if flg & 4 else 0
        return _lz4_clamp_hint(total, n)


def _lz4_clamp_hint(total, n):
        """No LZ4 input decodes to more than 255 bytes per byte (a match token followed by one length-extension byte after another), so the hint need not exceed
        that: a 100 KB frame of 20 000 one-byte blocks at 4 MiB would otherwise ask for 78 GiB.  A hint of 2 GiB or more is not one (None)."""
        if not total:
            return None
        total = min(total + 64, 255 * n + (1 << 16))
        return total if total < (1 << 31) else None


class LZ4Legacy(_FramedMany, _Format):
    """src/AuroraLib.Compression/Formats/Common/LZ4Legacy.cs"""
    container = A.C_LZ4_LEGACY
    provides_size = False

    def _capacity_hint(self, data):
        return _lz4_capacity_hint(data)


class Snappy(_FramedMany, _Format):
    """src/AuroraLib.Compression/Formats/Common/Snappy.cs (framing format, 64 KiB chunks)."""
    container = A.C_SNAPPY
    provides_size = False


class LZ40(_Format):
    """src/AuroraLib.Compression.Nintendo/Nintendo/LZ40.cs -- LZ11-like tokens, little endian, negated flag bytes."""
    container = A.C_LZ40


class LZ60(_Format):
    """src/AuroraLib.Compression.Nintendo/Nintendo/LZ60.cs -- identifier 0x60 over LZ40's body."""
    container = A.C_LZ60


class LZHudson(_Format):
    """src/AuroraLib.Compression.Nintendo/HudsonSoft/LZHudson.cs -- Yay0's grammar, one stream, 32-bit flag words."""
    container = A.C_LZHUDSON


class SMSR00(_Format):
    """src/AuroraLib.Compression.Nintendo/Nintendo/SMSR00.cs -- 16-bit masks + MIO0 tokens | literals."""
    container = A.C_SMSR00


class MDB4(_Format):
    """src/AuroraLib.Compression-Extended/Specialized/MDB4.cs"""
    container = A.C_MDB4


class FCMP(_Format):
    container = A.C_FCMP


class IECP(_Format):
    container = A.C_IECP


class GCZ(_Format):
    """Konami/GCZ.cs -- recognised by its file extension only, so IsMatch(data) is always False here."""
    container = A.C_GCZ


class ECD(_Format):
    """Specialized/ECD.cs -- 4 plain bytes + LZSS(10,6,2); stored when Quality == 0 or compression does not pay."""
    container = A.C_ECD


class SDPC(_Format):
    container = A.C_SDPC


HUF20_NO_ENCODER = ("HUF20 has no encoder here: the managed output is not a function of the input -- HuffmanTree.CreateTree orders equal frequencies "
                    "with the unstable List.Sort(), and the 4-bit path indexes its table with un-shifted high nibbles (DESIGN.md 7)")


class _NoHuffmanEncoder(_Format):
    """Compress of a Huffman type raises NotImplementedError with the reason (the library answers ALZ_E_UNSUPPORTED)."""
    huffman_types = ()

    def _is_huffman(self, settings):
        return self.Type in self.huffman_types

    def Compress(self, data, settings=None):
        if self._is_huffman(settings):
            raise NotImplementedError(HUF20_NO_ENCODER)
        return super().Compress(data, settings)


class RLE30(_Format):
    """src/AuroraLib.Compression.Nintendo/Nintendo/RLE30.cs -- 0x30 + size + run-length body (alz_rlh_*).  Compress keeps the managed
    defect: a literal run of 129 bytes (127 literals followed by fewer than 3 bytes) does not decode back."""
    container = A.C_RLE30


class HUF20(_NoHuffmanEncoder):
    """src/AuroraLib.Compression.Nintendo/Nintendo/HUF20.cs -- 0x24 / 0x28 + size + Huffman body (alz_rlh_*); decode only."""
    container = A.C_HUF20
    Huffman4bits, Huffman8bits = 0x24, 0x28

    def __init__(self):
        super().__init__()
        self.Type = self.Huffman8bits                 # HUF20.cs:37

    def _is_huffman(self, settings):
        return True


class LZ77(_NoHuffmanEncoder):
    """src/AuroraLib.Compression.Nintendo/Nintendo/LZ77.cs -- Type: LZ10 (default) / LZ11 / ChunkLZ10 / RLE30 / HUF20_4bits / HUF20_8bits (decode only)."""
    container = A.C_LZ77
    LZ10, LZ11, ChunkLZ10 = A.LZ77_LZ10, A.LZ77_LZ11, A.LZ77_CHUNKLZ10
    RLE30, HUF20_4bits, HUF20_8bits = A.LZ77_RLE30, A.LZ77_HUF20_4, A.LZ77_HUF20_8
    huffman_types = (A.LZ77_HUF20_4, A.LZ77_HUF20_8)


class Level5(_NoHuffmanEncoder):
    """src/AuroraLib.Compression.Nintendo/Level5/Level5.cs -- Type: OnlySave / LZ10 (default) / Huffman4Bit / Huffman8Bit (decode only) / RLE."""
    container = A.C_LEVEL5
    OnlySave, LZ10 = A.LEVEL5_ONLYSAVE, A.LEVEL5_LZ10
    Huffman4Bit, Huffman8Bit, RLE = A.LEVEL5_HUFFMAN4, A.LEVEL5_HUFFMAN8, A.LEVEL5_RLE
    huffman_types = (A.LEVEL5_HUFFMAN4, A.LEVEL5_HUFFMAN8)

    def _is_huffman(self, settings):
        return self.Type in self.huffman_types and not (settings is not None and settings.Quality == 0)   # quality 0 -> OnlySave first  Level5.cs:120-121


ALL_FORMATS = [LZSS, LZ10, LZ11, Yaz0, Yay0, MIO0, PRS, LZO, LZ4, LZ4Legacy, Snappy, GCLZ, CXLZ, LZ_3DS, COMP, Yaz1, AKLZ, LZ01, LZSega, Level5LZSS, LZOn, MDB4, FCMP, IECP, GCZ, ECD, SDPC, LZ40, LZ60, LZHudson, SMSR00, LZ00, FastLZ, CNX2, BLZ, CLZ0, CNS, LZ02, RefPack, WFLZ, LZShrek, HIG, LZ77, Level5, RLE30, HUF20]
__all__ = [c.__name__ for c in ALL_FORMATS] + ["CompressionSettings", "DecompressedSizeException", "EndOfStreamException", "InvalidIdentifierException", "InvalidDataException", "AlzError"]


APLIB_NO_ENCODER = ("aPLib has no encoder here: CompressHeaderless runs the tiered LzChainMatchFinder with a 2 MiB window and unbounded lengths, the bar is "
                    "bit-identity with the managed bytes checked against the CPU oracle, and the oracle has no aPLib (include/auroralz.h).  "
                    "Encode(data, settings) writes the file on the GPU: its bit-identity is held against a Python restatement of the finder that is "
                    "pinned to the oracle through other formats")


class _PrefixFile:
    """A class of the reference over its alz_<prefix>_* file entry points.  No alz_container value backs it, so it stays outside ALL_FORMATS."""
    prefix = None

    def _entry(self, what):
        return getattr(load(), "alz_%s_%s" % (self.prefix, what))

    def IsMatch(self, data):
        data = bytes(data)
        return bool(self._entry("is_match")(data, len(data)))


class _HeaderFile(_PrefixFile):
    """A header that states the size, around one body: alz_<prefix>_* reads the file, alz_<writer>_file_* writes it (Encode / EncodeMany; Compress
    still refuses) -- with a `kind` argument where the writer's family has several (alz_bitenc_*), without where it has one (alz_apenc_*)."""
    provides_size = True
    writer = None
    kind = None
    slot_floor = 0                        # EncodeMany: the least bytes a file's slot of the destination gets
    src_used_after = False                # Decompress: last_src_used is set only once the outcome has passed
    own_window = None                     # EncodeMany: why MaxWindowBits is refused

    def _aux0(self):
        return 0

    def _file_bound(self, n):
        return getattr(load(), "alz_%s_file_bound" % self.writer)(*(() if self.kind is None else (self.kind,)), n)

    def Encode(self, data, settings=None):
        """The file Compress of the reference writes for these settings (alz_apenc_file_compress / alz_bitenc_file_compress): the finder and the bit
        emitter on the GPU.  A lone large input goes through the batch pipeline -- there is no whole-GPU path for these formats.  Refused: MaxWindowBits
        other than 0; aPLib: an empty input (E_INVALID), and at qualities 1..7 an input longer than the managed chain table (2^18 bytes at quality 1,
        2^19 at 2..4, 2^20 at 5..7: E_UNSUPPORTED); ALLZ at quality 1 (E_UNSUPPORTED); a CRILAYLA source under 0x100 bytes (E_INVALID)."""
        data = bytes(data)
        st = _alz_settings(settings)
        head = (st,) if self.kind is None else (self.kind, st, self._aux0())
        return _single(getattr(load(), "alz_%s_file_compress" % self.writer), head, data, self._file_bound(len(data)))

    def EncodeMany(self, datas, settings=None):
        """Encode for a whole set of inputs in ONE alz_apenc_file_compress_batch / alz_bitenc_file_compress_batch (one encode batch).  Returns a list
        with, per input, the file's bytes -- or the exception instance Encode would have raised for it."""
        datas = [bytes(d) for d in datas]
        s = settings or CompressionSettings.Balanced
        if s.MaxWindowBits:
            raise AlzError(A.E_UNSUPPORTED, "MaxWindowBits %d: %s" % (s.MaxWindowBits, self.own_window))

        def run(table, src, dst_bytes):
            return getattr(_context(), "%s_file_compress_batch" % self.writer)(table, src, dst_bytes, s.Quality, s.Strategy)
        return _batch(datas, [max(self._file_bound(len(d)), self.slot_floor) for d in datas], run, self.kind or 0, self._aux0(),
                      entry="alz_%s_file_compress_batch" % self.writer)

    def GetDecompressedSize(self, data):
        data = bytes(data)
        size = C.c_uint32()
        rc = self._entry("decompressed_size")(data, len(data), C.byref(size))
        if rc == A.E_FORMAT:
            raise InvalidIdentifierException()
        check(rc)
        return size.value

    def Decompress(self, data, capacity=None):
        data = bytes(data)
        if capacity is None:
            capacity = self.GetDecompressedSize(data)
        return _single(self._entry("decompress"), (), data, capacity, _keeps_src_used(self), self.src_used_after)


class APLib(_HeaderFile):
    """src/AuroraLib.Compression/Formats/Common/aPLib.cs -- "AP32" + 24-byte header + body, or a headerless body (alz_aplib_*) and, for writing,
    alz_apenc_file_* (Encode / EncodeMany; Compress still refuses).  No alz_container value backs it, so it stays outside ALL_FORMATS."""
    prefix, writer = "aplib", "apenc"
    slot_floor = 1
    src_used_after = True
    own_window = "aPLib is written at its own window only"

    def MeasureDecompressedSize(self, data, limit=A.MEASURE_NO_BOUND):
        """The decoded size of a HEADERLESS body, counted on the GPU without decoding (alz_aplib_measure_batch)."""
        data = bytes(data)
        st = (A.Stream * 1)(A.Stream(0, 0, len(data), limit, 0, 0, 0, 0))
        r = _context().aplib_measure_batch(st, np.frombuffer(data + bytes(64), dtype=np.uint8))[0]
        _raise_for_outcome(A.E_STREAM if r.status else 0, r.status, r.dst_len)
        return r.dst_len

    def Decompress(self, data, capacity=None):
        """aPLib.Decompress: an "AP32" file, or -- without the magic -- a headerless body (whose size is measured first when no capacity is given)."""
        data = bytes(data)
        if capacity is None:
            capacity = self.GetDecompressedSize(data) if data[:4] == b"AP32" and len(data) >= 24 else self.MeasureDecompressedSize(data)
        return super().Decompress(data, capacity)

    def Compress(self, data, settings=None):
        raise NotImplementedError(APLIB_NO_ENCODER)


INFLATE_NO_ENCODER = ("%s has no encoder here: the reference hands Compress to the BCL, whose output depends on the zlib build behind it, "
                      "so there are no managed bytes to be bit-identical with (include/auroralz.h); Deflate / DeflateMany write the file with "
                      "the library's own DEFLATE encoder")


class _InflateFile(_PrefixFile):
    """A class of the reference that hands its body to the BCL, over its alz_<prefix>_* file entry points (alz_inflate_decode_batch underneath);
    decode only.  No alz_container value backs it, so it stays outside ALL_FORMATS.  The format stores no size in front of the data."""
    provides_size = False

    def MeasureDecompressedSize(self, data, limit=A.MEASURE_NO_BOUND):
        """The decoded size of the file, counted on the GPU without decoding (alz_<prefix>_measure); checksums are taken as correct."""
        data = bytes(data)
        n, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
        rc = self._entry("measure")(_context().h, data, len(data), limit, C.byref(n), C.byref(su), C.byref(st))
        _raise_for_outcome(rc, st.value, n.value)
        return n.value

    def Decompress(self, data, cap=None):
        """Decompress(Stream, Stream): with no `cap` the size is measured first."""
        data = bytes(data)
        if cap is None:
            cap = self.MeasureDecompressedSize(data)
        return _single(self._entry("decompress"), (), data, cap, _keeps_src_used(self))

    def DecompressMany(self, files, limit=A.MEASURE_NO_BOUND):
        """Decompress for a whole set of files in two GPU batches: one alz_zfile_measure_batch (sizes up to `limit`), a destination of exactly
        the measured sizes, one alz_zfile_decode_batch.  Returns a list with, per file, its bytes -- or the exception instance Decompress would
        have raised for it."""
        ctx = _context()
        return _decompress_many(files, self._kind(), limit, ctx.zfile_measure_batch, ctx.zfile_decode_batch)

    def Compress(self, data, settings=None):
        raise NotImplementedError(INFLATE_NO_ENCODER % type(self).__name__)

    # ---- the library's own encoder (alz_deflate_*): valid files of the class, not the bytes a BCL would write
    def _kind(self):
        return A.ZFILE_ZLIB if self.prefix == "zlib" else A.ZFILE_GZIP

    def DeflateLevel(self, settings=None):
        """(level, fixed): what the reference's Compress would hand the BCL for these settings."""
        raise NotImplementedError

    def Deflate(self, data, level=6, fixed=False):
        """The file of this class around a DEFLATE body of `level` 0..9 (alz_deflate_file_compress); fixed: fixed Huffman codes only."""
        data = bytes(data)
        lib, kind = load(), self._kind()
        return _single(lib.alz_deflate_file_compress, (kind, level, A.DEFLATE_FIXED if fixed else 0), data, lib.alz_deflate_file_bound(kind, len(data)))

    def DeflateMany(self, datas, level=6, fixed=False):
        """Deflate for a whole set of inputs in ONE alz_deflate_file_compress_batch.  Returns a list with, per input, the file's bytes -- or the
        exception instance Deflate would have raised for it."""
        datas = [bytes(d) for d in datas]
        lib, kind = load(), self._kind()

        def run(table, src, dst_bytes):
            return _context().deflate_file_compress_batch(table, src, dst_bytes, level, A.DEFLATE_FIXED if fixed else 0)
        return _batch(datas, [lib.alz_deflate_file_bound(kind, len(d)) for d in datas], run, kind, entry="alz_deflate_file_compress_batch")


class ZLib(_InflateFile):
    """src/AuroraLib.Compression/Formats/Common/ZLib.cs -- RFC 1950: CMF, FLG, a DEFLATE body, the Adler-32 of the output (alz_zlib_*)."""
    prefix = "zlib"

    def DeflateLevel(self, settings=None):
        """ZLib.cs:43-44: level = Quality * 8 / 15 rounded down, CompatibilityMode (Strategy bit 0) asks for fixed codes."""
        settings = settings or CompressionSettings.Balanced
        return settings.Quality * 8 // 15, bool(settings.Strategy & 1)


class GZip(_InflateFile):
    """src/AuroraLib.Compression/Formats/Common/GZip.cs -- RFC 1952: members of header, DEFLATE body, CRC-32 and ISIZE (alz_gzip_*)."""
    prefix = "gzip"

    def DeflateLevel(self, settings=None):
        """The explicit CompressionLevel operator (CompressionSettings.cs:65-73): NoCompression, Fastest, Optimal, SmallestSize; never fixed."""
        settings = settings or CompressionSettings.Balanced
        q = settings.Quality
        return (0 if q <= 2 else 1 if q <= 6 else 6 if q <= 9 else 9), False


class _WrappedFile:
    """A class of the reference that is a small header over a body the library decodes already (alz_wfile_*).  No alz_container value backs
    it, so it stays outside ALL_FORMATS (WRAPPED_FORMATS lists these).  Decompress decodes into the stated size + 64 when no capacity is given,
    so that an overlong body surfaces as DecompressedSizeException."""
    provides_size = True
    kind = None
    deflate = True                                    # the body is DEFLATE: Compress is the BCL's, Deflate writes the file

    def _opt(self):
        o = A.ContainerOptions()
        o.big_endian = 1 if getattr(self, "FormatByteOrder", "Little") == "Big" else 0
        o.chunk_size = int(getattr(self, "ChunkSize", 0) or getattr(self, "BlockSize", 0))
        o.variant = int(getattr(self, "Options", 0)) & 0xFFFFFFFF
        return o

    def IsMatch(self, data):
        data = bytes(data)
        return bool(load().alz_wfile_is_match(self.kind, data, len(data)))

    def GetDecompressedSize(self, data):
        data = bytes(data)
        v, o = C.c_uint32(), self._opt()
        rc = load().alz_wfile_decompressed_size(self.kind, C.byref(o), data, len(data), C.byref(v))
        _raise_for_outcome(rc, A.ST_INPUT_TRUNCATED, 0)
        return v.value

    def Walk(self, data):
        """alz_wfile_walk: (parts as (src_off, src_len, body, dst_len), stated size, flags)"""
        data = bytes(data)
        o, n, size, fl = self._opt(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        lib = load()
        rc = lib.alz_wfile_walk(self.kind, C.byref(o), data, len(data), None, 0, C.byref(n), C.byref(size), C.byref(fl))
        parts = (A.WfilePart * max(n.value, 1))()
        if rc == A.E_INVALID and n.value:
            rc = lib.alz_wfile_walk(self.kind, C.byref(o), data, len(data), parts, n.value, C.byref(n), C.byref(size), C.byref(fl))
        _raise_for_outcome(rc, A.ST_INPUT_TRUNCATED, 0)
        return [(p.src_off, p.src_len, p.body, p.dst_len) for p in parts[:n.value]], size.value, fl.value

    def Decompress(self, data, capacity=None):
        data = bytes(data)
        if capacity is None:
            capacity = self.GetDecompressedSize(data) + 64
        o = self._opt()

        def used(n):
            self.last_src_used = n
            if self.kind == A.WF_SSZL and len(data) >= 16:
                self.Options = int.from_bytes(data[12:16], "little")        # Decompress stores the file's Options  SSZL.cs:92
        return _single(load().alz_wfile_decompress, (self.kind, C.byref(o)), data, capacity, used)

    def DecompressMany(self, files):
        """Decompress for a whole set of files of this class in ONE alz_wfile_decode_batch.  Returns a list with, per file, its bytes -- or the
        exception instance Decompress would have raised for it."""
        files = [bytes(f) for f in files]
        lib, o = load(), self._opt()

        def slot(f):
            v = C.c_uint32()
            return v.value + 64 if lib.alz_wfile_decompressed_size(self.kind, C.byref(o), f, len(f), C.byref(v)) == 0 else 0
        return _batch(files, [slot(f) for f in files], lambda table, src, dst_bytes: _context().wfile_decode_batch(table, src, dst_bytes),
                      self.kind, o.big_endian, extra=64)

    def _write(self, data, settings, level, flags):
        data = bytes(data)
        lib, o = load(), self._opt()
        return _single(lib.alz_wfile_compress, (self.kind, C.byref(o), _alz_settings(settings), level, flags), data,
                       lib.alz_wfile_compress_bound(self.kind, C.byref(o), len(data)))

    def Compress(self, data, settings=None):
        if self.deflate:
            raise NotImplementedError(INFLATE_NO_ENCODER % type(self).__name__)
        return self._write(data, settings, 0, 0)

    def Deflate(self, data, level=6, fixed=False):
        """The file of this class around DEFLATE bodies of `level` 0..9 from the library's own encoder (alz_wfile_compress)."""
        if not self.deflate:
            raise NotImplementedError("%s has managed bytes: use Compress" % type(self).__name__)
        return self._write(data, None, level, A.DEFLATE_FIXED if fixed else 0)


class AsuraZlb(_WrappedFile):
    """src/AuroraLib.Compression-Extended/EA/AsuraZlb.cs"""
    kind = A.WF_ASURAZLB


class ZLB(_WrappedFile):
    """src/AuroraLib.Compression-Extended/Rare/ZLB.cs"""
    kind = A.WF_ZLB


class MDF0(_WrappedFile):
    """src/AuroraLib.Compression-Extended/Konami/MDF0.cs"""
    kind = A.WF_MDF0


class RareZip(_WrappedFile):
    """src/AuroraLib.Compression-Extended/Rare/RareZip.cs"""
    kind = A.WF_RAREZIP


class HWGZ(_WrappedFile):
    """src/AuroraLib.Compression-Extended/Specialized/HWGZ.cs -- ChunkSize, FormatByteOrder (default big)"""
    kind = A.WF_HWGZ

    def __init__(self):
        self.ChunkSize, self.FormatByteOrder = 0x10000, "Big"


class SSZL(_WrappedFile):
    """src/AuroraLib.Compression-Extended/Specialized/SSZL.cs -- Options (default Compressed | Encrypted)"""
    kind = A.WF_SSZL
    Compressed, UseGzip, Unknown, Encrypted = 0x1, 0x2, 0x10000, 0x80000000

    def __init__(self):
        self.Options = SSZL.Compressed | SSZL.Encrypted


class ZLWF(_WrappedFile):
    """src/AuroraLib.Compression-Extended/WayForward/ZLWF.cs -- BlockSize, FormatByteOrder (default big); N independent WFLZ files"""
    kind = A.WF_ZLWF
    deflate = False

    def __init__(self):
        self.BlockSize, self.FormatByteOrder = 0x400000, "Big"


class RLHudson(_WrappedFile):
    """src/AuroraLib.Compression.Nintendo/HudsonSoft/RLHudson.cs -- u32 BE size, u32 BE 5, the byte RLE of alz_rlhudson_*"""
    kind = A.WF_RLHUDSON
    deflate = False


WRAPPED_FORMATS = [AsuraZlb, ZLB, MDF0, RareZip, HWGZ, SSZL, ZLWF, RLHudson]

BITLZ_NO_ENCODER = ("%s has no encoder here: CompressHeaderless runs the LzChainMatchFinder, the bar is bit-identity with the managed bytes checked against "
                    "the CPU oracle, and there is no oracle body to hold bit-identity against (include/auroralz.h).  Encode(data, settings) writes the file "
                    "on the GPU: its bit-identity is held against a Python restatement of the finder that is pinned to the oracle through other formats")


class _BitLzFile(_HeaderFile):
    """A class of the .Extended assembly over its alz_<prefix>_* file entry points (alz_bitlz_decode_batch underneath) and, for writing,
    alz_bitenc_file_* (Encode / EncodeMany; Compress still refuses).  No alz_container value backs it, so it stays outside ALL_FORMATS."""
    writer = "bitenc"
    own_window = "CRILAYLA and ALLZ are written at their own windows only"

    def Compress(self, data, settings=None):
        raise NotImplementedError(BITLZ_NO_ENCODER % type(self).__name__)


class CRILAYLA(_BitLzFile):
    """src/AuroraLib.Compression-Extended/CRI/CRILAYLA.cs -- "CRILAYLA" + size + csize + body + 0x100 plain header bytes (alz_crilayla_*).
    Decompress returns size + 0x100 bytes: the header bytes first, the body -- decoded from its last byte down -- behind them."""
    prefix = "crilayla"
    kind = A.BITLZ_CRILAYLA


class ALLZ(_BitLzFile):
    """src/AuroraLib.Compression-Extended/Specialized/ALLZ.cs -- "ALLZ" + 4 flag bytes + size + body (alz_allz_*).  The three fields are
    what Compress would write into the header (ALLZ.cs:34-36); Decompress takes them from the file."""
    prefix = "allz"
    kind = A.BITLZ_ALLZ

    def _aux0(self):
        return A.allz_aux0(self.LzCopyBits, self.LzDistanceBits, self.LzLengthBits)

    def __init__(self):
        self.LzCopyBits, self.LzDistanceBits, self.LzLengthBits = 0, 10, 1
