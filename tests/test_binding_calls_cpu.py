"""No GPU: what the Python layer hands the C ABI.  A recording object stands in for libauroralz.so wherever a call takes a context: it notes the
function, the scalar arguments and the bytes of the stream table, and answers from a script of the test (per file an rc / status / dst_len and a
byte pattern at the file's dst_off).  Functions that are host arithmetic (*_bound, *_is_match, *_decompressed_size) go to the built library.
Stated by hand for three inputs of 0, 1 and 17 bytes, the middle one scripted to fail: the table rows and destination sizes of the batch methods
of formats.py, the two calls behind every DecompressMany, what comes back per file, and when the single-file readers set last_src_used.  Last,
the loaded library carries exactly the prototypes of _abi.PROTOTYPES, and they are the header's."""
import ctypes as C
import os
import re

import pytest

import test_shim_binding as SB
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import _lib
from auroralib.compression_amd import batch
from auroralib.compression_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = 0x5EED
INPUTS = [b"", b"\x07", bytes(range(17))]
HOST_ARITHMETIC = re.compile(r"alz_\w+_(bound|is_match|decompressed_size)$")
OK, FAILS = (0, A.ST_OK), (A.E_INVALID, A.ST_OK)


def pattern(i, n):
    """what the stand-in leaves at dst_off of file i"""
    return bytes([0xA0 + i]) * n


class Recorder:
    """libauroralz.so for the calls that take a context.  scripts: one per expected call, in order -- for a batch a list of (rc, status, dst_len)
    per file, for a single-file call a dict of rc / dl / su / st."""

    def __init__(self, *scripts):
        self.real, self.scripts, self.calls, self.host = _lib.load(), list(scripts), [], {}

    def __getattr__(self, name):
        if HOST_ARITHMETIC.match(name):
            return self.host.get(name) or getattr(self.real, name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        assert isinstance(args[0], C.c_void_p) and args[0].value == HANDLE, name
        args = [a._obj if type(a).__name__ == "CArgObject" else a for a in args[1:]]            # (byref(x) -> x)
        call = {"fn": name, "scalars": [], "table": None, "data": None}
        ptrs, outs, status, table, results = [], [], None, None, None
        for a in args:
            if a is None or isinstance(a, int):
                call["scalars"].append(a)
            elif isinstance(a, A.Settings):
                call["scalars"].append(("settings", a.quality, a.max_window_bits, a.strategy, a.min_distance))
            elif isinstance(a, A.ContainerOptions):
                call["scalars"].append(("options", a.big_endian, a.variant, a.chunk_size))
            elif isinstance(a, bytes):
                call["data"] = a
            elif isinstance(a, C.Array) and a._type_ is A.Stream:
                table, call["table"] = a, bytes(a)
            elif isinstance(a, C.Array) and a._type_ is A.FileResult:
                results = a
            elif isinstance(a, C.c_void_p):
                ptrs.append(a.value)
            elif isinstance(a, C.c_size_t):
                outs.append(a)
            elif isinstance(a, C.c_int32):
                status = a
            else:
                raise AssertionError("%s: an argument of %r" % (name, type(a)))
        self.calls.append(call)
        script = self.scripts.pop(0)
        if results is not None:                                                                    # a batch over a file table
            assert len(script) == len(table) == len(results), name
            for i, (rc, st, n) in enumerate(script):
                results[i].rc, results[i].status, results[i].dst_len, results[i].src_used = rc, st, n, table[i].src_len
                if len(ptrs) == 2:                                                                 # (src, dst; the last scalar is dst_bytes)
                    assert table[i].dst_off + n <= call["scalars"][-1] and n <= table[i].dst_cap, (name, i)
                    C.memmove(ptrs[1] + table[i].dst_off, pattern(i, n), n)
            return 0
        assert len(ptrs) == 1 and script["dl"] <= call["scalars"][-1], name                        # one file: dst; the last scalar is its capacity
        C.memmove(ptrs[0], pattern(0, script["dl"]), script["dl"])
        outs[0].value = script["dl"]
        if status is not None:
            outs[1].value, status.value = script["su"], script["st"]
        return script["rc"]


@pytest.fixture
def stand_in(monkeypatch):
    def make(*scripts):
        rec = Recorder(*scripts)
        ctx = object.__new__(batch.Context)
        ctx.lib, ctx.h, ctx.device = rec, C.c_void_p(HANDLE), 0
        monkeypatch.setattr(F, "load", lambda: rec)
        monkeypatch.setattr(F, "_ctx", ctx)
        return rec
    return make


def rows(*r):
    """the bytes of a stream table from (src_off, dst_off, src_len, dst_cap, aux0, format) per file"""
    return bytes((A.Stream * len(r))(*[A.Stream(so, do, sl, cap, 0, aux0, 0, fmt) for so, do, sl, cap, aux0, fmt in r]))


def check_files(out, lens, entry):
    """files 0 and 2 are the stand-in's patterns, file 1 the error of the entry point"""
    assert [type(o) for o in out] == [bytes, F.AlzError, bytes]
    assert out[0] == pattern(0, lens[0]) and out[2] == pattern(2, lens[2])
    assert out[1].code == A.E_INVALID and str(out[1]) == "auroralz error %d: %s: file 1" % (A.E_INVALID, entry)


# ---------------------------------------------------------------------------------------------- the batch methods: one call each
def test_compress_many_packs_slots_back_to_back(stand_in):
    """no alignment of dst_off: the slots are the bounds, one behind the other; aux0 is the block size"""
    lib = _lib.load()
    caps = [lib.alz_container_compress_bound(A.C_LZ4_FRAME, n) for n in (0, 1, 17)]
    assert caps == [72, 73, 89] and caps[0] % 16 and (caps[0] + caps[1]) % 16                       # (so that an alignment would show)
    rec = stand_in([OK + (5,), FAILS + (0,), OK + (9,)])
    out = F.LZ4(F.LZ4.Block64KB).CompressMany(INPUTS, F.CompressionSettings(12, 3, 1))
    assert len(rec.calls) == 1 and rec.calls[0]["fn"] == "alz_framing_compress_batch"
    assert rec.calls[0]["scalars"] == [("settings", 12, 3, 1, 0), 3, 19, 72 + 73 + 89]
    assert rec.calls[0]["table"] == rows((0, 0, 0, 72, 0x10000, A.C_LZ4_FRAME), (0, 72, 1, 73, 0x10000, A.C_LZ4_FRAME), (1, 145, 17, 89, 0x10000, A.C_LZ4_FRAME))
    check_files(out, (5, 0, 9), "alz_framing_compress_batch")


def test_aplib_encode_many_rounds_every_slot_to_16(stand_in):
    lib = _lib.load()
    assert [lib.alz_apenc_file_bound(n) for n in (0, 1, 17)] == [24, 27, 45]
    rec = stand_in([OK + (24,), FAILS + (0,), OK + (45,)])
    out = F.APLib().EncodeMany(INPUTS, F.CompressionSettings(4, 0, 1))
    assert len(rec.calls) == 1 and rec.calls[0]["fn"] == "alz_apenc_file_compress_batch"
    assert rec.calls[0]["scalars"] == [("settings", 4, 0, 1, 0), 3, 19, 32 + 32 + 48]
    assert rec.calls[0]["table"] == rows((0, 0, 0, 24, 0, 0), (0, 32, 1, 27, 0, 0), (1, 64, 17, 45, 0, 0))
    check_files(out, (24, 0, 45), "alz_apenc_file_compress_batch")


def test_aplib_slot_floor_is_one_byte(stand_in):
    """max(bound, 1): were the bound 0, a file would still get a slot of one byte (and 16 bytes of the destination)"""
    rec = stand_in([OK + (1,), OK + (0,)])
    rec.host["alz_apenc_file_bound"] = lambda n: 0
    assert F.APLib().EncodeMany([b"ab", b"c"]) == [pattern(0, 1), b""]
    assert rec.calls[0]["scalars"][1:] == [2, 4, 32] and rec.calls[0]["table"] == rows((0, 0, 2, 1, 0, 0), (2, 16, 1, 1, 0, 0))


@pytest.mark.parametrize("cls,kind,aux0", [(F.CRILAYLA, A.BITLZ_CRILAYLA, 0), (F.ALLZ, A.BITLZ_ALLZ, A.allz_aux0(0, 10, 1))])
def test_bitlz_encode_many_rounds_every_slot_to_16(stand_in, cls, kind, aux0):
    caps, up = ([0, 0, 0], [0, 0, 0]) if kind == A.BITLZ_CRILAYLA else ([28, 29, 119], [32, 32, 128])    # (a CRILAYLA source under 0x100 bytes is refused: no slot)
    assert caps == [_lib.load().alz_bitenc_file_bound(kind, n) for n in (0, 1, 17)]
    rec = stand_in([OK + (min(3, caps[0]),), FAILS + (0,), OK + (caps[2],)])
    out = cls().EncodeMany(INPUTS, F.CompressionSettings(10, 0, 1))
    assert len(rec.calls) == 1 and rec.calls[0]["fn"] == "alz_bitenc_file_compress_batch"
    assert rec.calls[0]["scalars"] == [("settings", 10, 0, 1, 0), 3, 19, up[0] + up[1] + up[2]]
    assert rec.calls[0]["table"] == rows((0, 0, 0, caps[0], aux0, kind), (0, up[0], 1, caps[1], aux0, kind), (1, up[0] + up[1], 17, caps[2], aux0, kind))
    check_files(out, (min(3, caps[0]), 0, caps[2]), "alz_bitenc_file_compress_batch")


@pytest.mark.parametrize("cls,kind", [(F.ZLib, A.ZFILE_ZLIB), (F.GZip, A.ZFILE_GZIP)])
def test_deflate_many_rounds_every_slot_to_16(stand_in, cls, kind):
    caps, up = ([11, 12, 28], [16, 16, 32]) if kind == A.ZFILE_ZLIB else ([23, 24, 40], [32, 32, 48])
    assert caps == [_lib.load().alz_deflate_file_bound(kind, n) for n in (0, 1, 17)]
    rec = stand_in([OK + (2,), FAILS + (0,), OK + (caps[2],)])
    out = cls().DeflateMany(INPUTS, level=9, fixed=True)
    assert len(rec.calls) == 1 and rec.calls[0]["fn"] == "alz_deflate_file_compress_batch"
    assert rec.calls[0]["scalars"] == [9, A.DEFLATE_FIXED, 3, 19, up[0] + up[1] + up[2]]
    assert rec.calls[0]["table"] == rows((0, 0, 0, caps[0], 0, kind), (0, up[0], 1, caps[1], 0, kind), (1, up[0] + up[1], 17, caps[2], 0, kind))
    check_files(out, (2, 0, caps[2]), "alz_deflate_file_compress_batch")


def rlhudson_file(size, n):
    """n bytes that state `size`: u32 BE size, u32 BE 5, body"""
    return (size.to_bytes(4, "big") + (5).to_bytes(4, "big") + bytes(n))[:n]


def test_wrapped_decompress_many_adds_64_to_the_size_and_to_the_total(stand_in):
    """a slot is the stated size + 64 (0 where the header does not give one), rounded to 16 in the layout; the destination is 64 bytes longer;
    a failed file is the exception Decompress raises"""
    files = [b"", b"\x00", rlhudson_file(40, 17)]
    rec = stand_in([(A.E_FORMAT, A.ST_OK, 0), (A.E_STREAM, A.ST_INPUT_TRUNCATED, 0), OK + (40,)])
    out = F.RLHudson().DecompressMany(files)
    assert len(rec.calls) == 1 and rec.calls[0]["fn"] == "alz_wfile_decode_batch"
    assert rec.calls[0]["scalars"] == [3, 19, 112 + 64]
    assert rec.calls[0]["table"] == rows((0, 0, 0, 0, 0, A.WF_RLHUDSON), (0, 0, 1, 0, 0, A.WF_RLHUDSON), (1, 0, 17, 104, 0, A.WF_RLHUDSON))
    assert [type(o) for o in out] == [F.InvalidIdentifierException, F.EndOfStreamException, bytes] and out[2] == pattern(2, 40)
    rec = stand_in([OK + (40,), (A.E_STREAM, A.ST_OUTPUT_SIZE_MISMATCH, 7), OK + (3,)])             # three good headers: every start on a multiple of 16
    out = F.RLHudson().DecompressMany([rlhudson_file(40, 17), rlhudson_file(1, 9), rlhudson_file(3, 17)])
    assert rec.calls[0]["scalars"] == [3, 44, 112 + 80 + 80 + 64]
    assert rec.calls[0]["table"] == rows((0, 0, 17, 104, 0, A.WF_RLHUDSON), (17, 112, 9, 65, 0, A.WF_RLHUDSON), (26, 192, 17, 67, 0, A.WF_RLHUDSON))
    assert out[0] == pattern(0, 40) and type(out[1]) is F.DecompressedSizeException and out[1].args == (7,) and out[2] == pattern(2, 3)


def test_wrapped_decompress_many_hands_over_the_byte_order(stand_in):
    hw = F.HWGZ()
    rec = stand_in([(A.E_FORMAT, A.ST_OK, 0)])
    assert type(hw.DecompressMany([b"abc"])[0]) is F.InvalidIdentifierException
    assert rec.calls[0]["table"] == rows((0, 0, 3, 0, 1, A.WF_HWGZ))
    hw.FormatByteOrder = "Little"
    rec = stand_in([(A.E_FORMAT, A.ST_OK, 0)])
    hw.DecompressMany([b"abc"])
    assert rec.calls[0]["table"] == rows((0, 0, 3, 0, 0, A.WF_HWGZ))


# ---------------------------------------------------------------------------------------------- DecompressMany: measure, then decode the good ones
TRUNCATED, CAPACITY = (A.E_STREAM, A.ST_INPUT_TRUNCATED), (A.E_STREAM, A.ST_OUTPUT_CAPACITY)


def test_decompress_many_decodes_only_what_measured_well(stand_in):
    """zlib / gzip: a file whose measure failed is not decoded; the decode table has the measured sizes back to back (no alignment)"""
    rec = stand_in([OK + (5,), TRUNCATED + (3,), OK + (7,)], [OK + (5,), OK + (7,)])
    out = F.GZip().DecompressMany(INPUTS, limit=1000)
    assert [c["fn"] for c in rec.calls] == ["alz_zfile_measure_batch", "alz_zfile_decode_batch"]
    assert rec.calls[0]["scalars"] == [3, 19] and rec.calls[1]["scalars"] == [2, 19, 12]
    assert rec.calls[0]["table"] == rows((0, 0, 0, 1000, 0, A.ZFILE_GZIP), (0, 0, 1, 1000, 0, A.ZFILE_GZIP), (1, 0, 17, 1000, 0, A.ZFILE_GZIP))
    assert rec.calls[1]["table"] == rows((0, 0, 0, 5, 0, A.ZFILE_GZIP), (1, 5, 17, 7, 0, A.ZFILE_GZIP))
    assert out[0] == pattern(0, 5) and type(out[1]) is F.EndOfStreamException and out[2] == pattern(1, 7)
    rec = stand_in([OK + (5,), TRUNCATED + (3,), OK + (7,)], [OK + (5,), (A.E_CHECKSUM, A.ST_OK, 7)])
    out = F.ZLib().DecompressMany(INPUTS)
    assert rec.calls[0]["table"] == rows((0, 0, 0, A.MEASURE_NO_BOUND, 0, A.ZFILE_ZLIB), (0, 0, 1, A.MEASURE_NO_BOUND, 0, A.ZFILE_ZLIB), (1, 0, 17, A.MEASURE_NO_BOUND, 0, A.ZFILE_ZLIB))
    assert out[0] == pattern(0, 5) and type(out[1]) is F.EndOfStreamException and type(out[2]) is F.InvalidDataException


def test_decompress_many_lets_the_decode_decide_a_stream_error(stand_in):
    """LZ4 / Snappy files (decode_decides): a measure that ends in a stream error other than the limit is decoded as well, into what it measured"""
    rec = stand_in([OK + (5,), TRUNCATED + (3,), OK + (7,)], [OK + (5,), (A.E_CHECKSUM, A.ST_OK, 3), OK + (7,)])
    out = F.LZ4().DecompressMany(INPUTS, limit=1000)
    assert [c["fn"] for c in rec.calls] == ["alz_framed_measure_batch", "alz_framed_decode_batch"]
    assert rec.calls[0]["scalars"] == [3, 19] and rec.calls[1]["scalars"] == [3, 19, 15]
    assert rec.calls[0]["table"] == rows((0, 0, 0, 1000, 0, A.C_LZ4_FRAME), (0, 0, 1, 1000, 0, A.C_LZ4_FRAME), (1, 0, 17, 1000, 0, A.C_LZ4_FRAME))
    assert rec.calls[1]["table"] == rows((0, 0, 0, 5, 0, A.C_LZ4_FRAME), (0, 5, 1, 3, 0, A.C_LZ4_FRAME), (1, 8, 17, 7, 0, A.C_LZ4_FRAME))
    assert out[0] == pattern(0, 5) and type(out[1]) is F.InvalidDataException and out[2] == pattern(2, 7)
    rec = stand_in([OK + (5,), CAPACITY + (1000,), OK + (7,)], [OK + (5,), OK + (7,)])            # the limit itself: not decoded
    out = F.Snappy().DecompressMany(INPUTS, limit=1000)
    assert rec.calls[1]["scalars"] == [2, 19, 12] and rec.calls[1]["table"] == rows((0, 0, 0, 5, 0, A.C_SNAPPY), (1, 5, 17, 7, 0, A.C_SNAPPY))
    assert out[0] == pattern(0, 5) and type(out[1]) is BufferError and out[2] == pattern(1, 7)
    rec = stand_in([(A.E_FORMAT, A.ST_OK, 0)] * 3)                                                  # nothing measured well: no second call
    assert [type(o) for o in F.LZ4Legacy().DecompressMany(INPUTS)] == [F.InvalidIdentifierException] * 3 and len(rec.calls) == 1


# ---------------------------------------------------------------------------------------------- no inputs
def test_empty_lists(stand_in):
    """CompressMany and the two-batch DecompressMany make no call for an empty list; the other four make theirs with n = 0, one byte of source"""
    rec = stand_in()
    assert F.Snappy().CompressMany([]) == [] and F.LZ4().DecompressMany([]) == [] and F.ZLib().DecompressMany([]) == [] and rec.calls == []
    for run, fn, scalars in ((lambda: F.APLib().EncodeMany([]), "alz_apenc_file_compress_batch", [("settings", 8, 0, 0, 0), 0, 1, 0]),
                             (lambda: F.ALLZ().EncodeMany([]), "alz_bitenc_file_compress_batch", [("settings", 8, 0, 0, 0), 0, 1, 0]),
                             (lambda: F.GZip().DeflateMany([]), "alz_deflate_file_compress_batch", [6, 0, 0, 1, 0]),
                             (lambda: F.ZLB().DecompressMany([]), "alz_wfile_decode_batch", [0, 1, 64])):
        rec = stand_in([])
        assert run() == [] and [c["fn"] for c in rec.calls] == [fn] and rec.calls[0]["scalars"] == scalars and rec.calls[0]["table"] == b"", fn


def test_encode_many_refuses_a_window_before_anything_is_packed(stand_in):
    rec = stand_in()
    for cls, text in ((F.APLib, "aPLib is written at its own window only"), (F.CRILAYLA, "CRILAYLA and ALLZ are written at their own windows only")):
        with pytest.raises(F.AlzError) as e:
            cls().EncodeMany(INPUTS, F.CompressionSettings(8, 12))
        assert e.value.code == A.E_UNSUPPORTED and str(e.value) == "auroralz error %d: MaxWindowBits 12: %s" % (A.E_UNSUPPORTED, text)
    assert rec.calls == []


# ---------------------------------------------------------------------------------------------- one file
def readers():
    sszl = F.SSZL()
    return [(F.LZ10(), "alz_container_decompress", [A.C_LZ10, ("options", 1, 0, 0)], False), (F.APLib(), "alz_aplib_decompress", [], False),
            (F.GZip(), "alz_gzip_decompress", [], True), (F.CRILAYLA(), "alz_crilayla_decompress", [], True), (F.ALLZ(), "alz_allz_decompress", [], True),
            (F.RLHudson(), "alz_wfile_decompress", [A.WF_RLHUDSON, ("options", 0, 0, 0)], True),
            (sszl, "alz_wfile_decompress", [A.WF_SSZL, ("options", 0, sszl.Options, 0)], True)]


@pytest.mark.parametrize("case", range(7))
def test_readers_set_last_src_used_when_they_always_did(stand_in, case):
    """a failed call: the readers of ZLib / GZip, CRILAYLA / ALLZ and the wrapped files have noted the source bytes used before the outcome is
    raised (and SSZL the file's Options), the container classes and aPLib have not; a good call: all have, and the bytes are the first dst_len of
    the destination"""
    data = bytes(range(1, 18))
    obj, fn, lead, noted_on_failure = readers()[case]
    rec = stand_in({"rc": A.E_STREAM, "st": A.ST_INPUT_TRUNCATED, "dl": 2, "su": 9})
    with pytest.raises(F.EndOfStreamException):
        obj.Decompress(data, 33)
    assert [c["fn"] for c in rec.calls] == [fn] and rec.calls[0]["scalars"] == lead + [17, 33] and rec.calls[0]["data"] == data
    assert getattr(obj, "last_src_used", None) == (9 if noted_on_failure else None)
    if isinstance(obj, F.SSZL):
        assert obj.Options == int.from_bytes(data[12:16], "little")
    obj = readers()[case][0]
    rec = stand_in({"rc": 0, "st": A.ST_OK, "dl": 30, "su": 17})
    assert obj.Decompress(data, 33) == pattern(0, 30) and obj.last_src_used == 17
    rec = stand_in({"rc": 0, "st": A.ST_OK, "dl": 0, "su": 1})                                      # a capacity of 0 is handed on as 0 (the array behind it has one byte)
    assert obj.Decompress(data, 0) == b"" and rec.calls[0]["scalars"][-2:] == [17, 0]


def writers():
    s = F.CompressionSettings(12, 3, 1)
    lib = _lib.load()
    opt = A.ContainerOptions()
    return [(lambda: F.LZ10().Compress(DATA, s), "alz_container_compress", [A.C_LZ10, ("options", 1, 0, 0), ("settings", 12, 3, 1, 0)], lib.alz_container_compress_bound(A.C_LZ10, 17)),
            (lambda: F.APLib().Encode(DATA, s), "alz_apenc_file_compress", [("settings", 12, 3, 1, 0)], lib.alz_apenc_file_bound(17)),
            (lambda: F.ALLZ().Encode(DATA, s), "alz_bitenc_file_compress", [A.BITLZ_ALLZ, ("settings", 12, 3, 1, 0), A.allz_aux0(0, 10, 1)], lib.alz_bitenc_file_bound(A.BITLZ_ALLZ, 17)),
            (lambda: F.CRILAYLA().Encode(DATA, s), "alz_bitenc_file_compress", [A.BITLZ_CRILAYLA, ("settings", 12, 3, 1, 0), 0], lib.alz_bitenc_file_bound(A.BITLZ_CRILAYLA, 17)),
            (lambda: F.ZLib().Deflate(DATA, 9, True), "alz_deflate_file_compress", [A.ZFILE_ZLIB, 9, A.DEFLATE_FIXED], lib.alz_deflate_file_bound(A.ZFILE_ZLIB, 17)),
            (lambda: F.RLHudson().Compress(DATA, s), "alz_wfile_compress", [A.WF_RLHUDSON, ("options", 0, 0, 0), ("settings", 12, 3, 1, 0), 0, 0],
             lib.alz_wfile_compress_bound(A.WF_RLHUDSON, C.byref(opt), 17)),
            (lambda: F.ZLB().Deflate(DATA, 3, True), "alz_wfile_compress", [A.WF_ZLB, ("options", 0, 0, 0), ("settings", 8, 0, 0, 0), 3, A.DEFLATE_FIXED],
             lib.alz_wfile_compress_bound(A.WF_ZLB, C.byref(opt), 17))]


DATA = bytes(range(1, 18))


@pytest.mark.parametrize("case", range(7))
def test_writers_hand_over_the_bound_and_return_the_bytes_written(stand_in, case):
    run, fn, lead, cap = writers()[case]
    n = min(11, cap)                                                                               # (a CRILAYLA source under 0x100 bytes has a bound of 0)
    rec = stand_in({"rc": 0, "dl": n})
    assert run() == pattern(0, n)
    assert [c["fn"] for c in rec.calls] == [fn] and rec.calls[0]["scalars"] == lead + [17, cap] and rec.calls[0]["data"] == DATA
    stand_in({"rc": A.E_UNSUPPORTED, "dl": 0})
    with pytest.raises(F.AlzError) as e:
        run()
    assert e.value.code == A.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the prototypes
def test_loaded_prototypes_are_the_table_and_the_table_is_the_header(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)                                                        # (a fresh load: function objects no other test has touched)
    lib = _lib.load()
    for name, types in A.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert (fn.argtypes or []) == types, name
        assert fn.restype is A.RESTYPES.get(name, C.c_int), name
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "auroralz.h")).read(), flags=re.S)
    declared = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"^\s*(int|void|size_t|uint32_t|const char\*)\s+(alz_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)}
    assert sorted(declared) == sorted(A.PROTOTYPES)
    returns = {"size_t": C.c_size_t, "uint32_t": C.c_uint32, "const char*": C.c_char_p, "void": None, "int": C.c_int}
    scalars = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
    for name, (ret, params) in declared.items():
        assert A.RESTYPES.get(name, C.c_int) is returns[ret], name
        want = SB._c_param_types(params)
        assert len(A.PROTOTYPES[name]) == len(want), name
        for ct, t in zip(want, A.PROTOTYPES[name]):                                                # a scalar is its ctypes twin, a pointer some pointer type
            assert (t is scalars[ct]) if ct in scalars else (ct.endswith("*") and (t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer))), (name, ct, t)
    assert lib.alz_container_compress_bound.restype is C.c_size_t                                  # (before any Compress of this process, too: load() sets it)
    assert lib.alz_container_compress_bound(A.C_LZ10, 1 << 33) > 1 << 33
    for name in ("alz_container_is_match", "alz_container_decompressed_size", "alz_container_compress", "alz_container_decompress", "alz_device_count", "alz_abi_version"):
        assert name in A.CONTAINER_PROTOTYPES or name in A.CORE_PROTOTYPES, name
