"""ctypes mirror of include/auroralz.h (POD structs, enums).  No logic here."""
import ctypes as C

ABI_VERSION = 2

# alz_format
FMT_LZSS, FMT_LZ10, FMT_LZ11, FMT_YAZ0, FMT_YAY0, FMT_MIO0, FMT_PRS_BE, FMT_PRS_LE, FMT_LZ4_BLOCK, FMT_LZO, FMT_SNAPPY_RAW, FMT_LZ40, FMT_LZHUDSON, FMT_SMSR00, FMT_FASTLZ, FMT_CNX2, FMT_BLZ, FMT_CLZ0, FMT_CNS, FMT_LZ02, FMT_REFPACK, FMT_WFLZ, FMT_WFLZ_BE, FMT_LZSHREK, FMT_HIG = range(25)
FMT_COUNT = 25
FORMAT_NAMES = ["lzss", "lz10", "lz11", "yaz0", "yay0", "mio0", "prs_be", "prs_le", "lz4_block", "lzo", "snappy_raw", "lz40", "lzhudson", "smsr00", "fastlz", "cnx2", "blz", "clz0", "cns", "lz02", "refpack", "wflz", "wflz_be", "lzshrek", "hig"]

# alz_status
ST_OK, ST_INPUT_TRUNCATED, ST_OUTPUT_SIZE_MISMATCH, ST_OUTPUT_CAPACITY, ST_BAD_TOKEN = range(5)

# API errors
E_INVALID, E_NO_DEVICE, E_HIP, E_NOMEM, E_UNSUPPORTED, E_FORMAT, E_STREAM, E_CHECKSUM = -1, -2, -3, -4, -5, -6, -7, -8

# alz_container
C_LZSS, C_LZ10, C_LZ11, C_YAZ0, C_YAY0, C_MIO0, C_PRS, C_LZ4_LEGACY, C_LZO, C_SNAPPY = range(10)
C_GCLZ, C_CXLZ, C_LZ_3DS, C_COMP, C_YAZ1, C_AKLZ, C_LZ01, C_LZSEGA, C_LEVEL5LZSS, C_LZON, C_LZ77, C_LEVEL5 = range(10, 22)
C_LZ4_FRAME = 22
C_MDB4, C_FCMP, C_IECP, C_GCZ, C_ECD, C_SDPC, C_LZ40, C_LZ60, C_LZHUDSON, C_SMSR00 = range(23, 33)
C_LZ00 = 33
C_FASTLZ = 34
C_CNX2 = 35
C_BLZ = 36
C_CLZ0 = 37
C_CNS = 38
C_LZ02 = 39
C_REFPACK = 40
C_WFLZ = 41
C_LZSHREK = 42
C_HIG = 43
C_RLE30 = 44
C_HUF20 = 45
C_COUNT = 46
LZ77_LZ10, LZ77_LZ11, LZ77_CHUNKLZ10 = 0x10, 0x11, 0xF7
LZ77_HUF20_4, LZ77_HUF20_8, LZ77_RLE30 = 0x24, 0x28, 0x30
LEVEL5_ONLYSAVE, LEVEL5_LZ10 = 0, 1
LEVEL5_HUFFMAN4, LEVEL5_HUFFMAN8, LEVEL5_RLE = 2, 3, 4

# alz_rlh_format: the non-LZ bodies of the GBA / DS family (an entry-point family of their own, not alz_format values)
RLH_RLE30, RLH_HUF20_4, RLH_HUF20_8 = range(3)
RLH_COUNT = 3
RLH_NAMES = ["rle30", "huf20_4", "huf20_8"]
HUF20_MAX_DECOM = 0x10000000           # decom_len from here on is refused (the managed int symbol count overflows)


class LzProperties(C.Structure):
    """alz_lz_properties == LzProperties (src/AuroraLib.Compression/LzProperties.cs:9-97)."""
    _fields_ = [("window_bits", C.c_uint8), ("length_bits", C.c_uint8), ("min_length", C.c_uint8), ("reserved0", C.c_uint8),
                ("windows_start", C.c_uint32), ("max_distance", C.c_uint32), ("reserved1", C.c_uint32)]

    @classmethod
    def from_bits(cls, distance_bits, length_bits, threshold=2):
        """LzProperties(byte distanceBits, byte lengthBits, byte threshold) -- LzProperties.cs:57-66."""
        md = 1 << distance_bits
        return cls(distance_bits, length_bits, threshold + 1, 0, md - (1 << length_bits) - threshold, md, 0)


class Stream(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("dst_off", C.c_uint64), ("src_len", C.c_uint32), ("dst_cap", C.c_uint32),
                ("decom_len", C.c_uint32), ("aux0", C.c_uint32), ("aux1", C.c_uint32), ("format", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("dst_len", C.c_uint32), ("src_used", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_uint32)]


class Settings(C.Structure):
    """alz_settings == CompressionSettings (src/AuroraLib.Compression/CompressionSettings.cs:11-84)."""
    _fields_ = [("quality", C.c_int32), ("max_window_bits", C.c_int32), ("strategy", C.c_int32), ("min_distance", C.c_int32)]


class EncodeAux(C.Structure):
    _fields_ = [("aux0", C.c_uint32), ("aux1", C.c_uint32)]


class ContainerOptions(C.Structure):
    _fields_ = [("big_endian", C.c_uint32), ("memory_alignment", C.c_uint32), ("lz", LzProperties), ("variant", C.c_uint32), ("chunk_size", C.c_uint32),
                ("key", C.c_uint32), ("name", C.c_uint8 * 32)]


_VP, _U32, _SZ, _VPP = C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_void_p)
_U32P, _SZP, _I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)

# Every function of include/auroralz.h has its argument types in one <FAMILY>_PROTOTYPES table below, and its return type in <FAMILY>_RESTYPES where
# that is not int; PROTOTYPES / RESTYPES at the end of the file join the tables, and _lib.load() applies them.

# the core: library and context, LZ batches on host and device buffers, plans, device memory
CORE_PROTOTYPES = {
    "alz_abi_version": [], "alz_device_count": [], "alz_last_error": [],
    "alz_create": [C.c_int, _VPP], "alz_destroy": [_VP],
    "alz_device_info": [_VP, C.c_char_p, _SZ, C.POINTER(C.c_int), C.POINTER(C.c_uint64)],
    "alz_ctx_set_exact_kernels": [_VP, C.c_int], "alz_ctx_set_kernel_variant": [_VP, C.c_int],
    "alz_ctx_big_stream": [_VP, _U32, C.POINTER(C.c_uint64)], "alz_ctx_release_scratch": [_VP],
    "alz_decode_batch": [_VP, _VP, _U32, _VP, _SZ, _VP, _VP, _SZ, _VP],
    "alz_decode_batch_multi": [_VPP, _U32, _VP, _U32, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP],
    "alz_partition_batch": [_U32, _VP, _U32, _VP, _VP],
    "alz_decode": [_VP, _U32, _VP, _VP, _U32, _U32, _U32, _U32, _VP, _U32, _VP],
    "alz_plan_create": [_VP, _VP, _U32, _VP, _VPP], "alz_plan_execute": [_VP, _VP, _VP, _VP, _VP],
    "alz_plan_execute_timed": [_VP, _VP, _VP, _VP, C.c_int, C.POINTER(C.c_float)],
    "alz_plan_results": [_VP, _VP, _VP], "alz_plan_destroy": [_VP, _VP],
    "alz_plan_create_multi": [_VP, _U32, _VP, _U32, _VP, _VP, _VPP, _VP], "alz_plan_execute_multi": [_VP, _VP, _VP],
    "alz_plan_results_multi": [_VP, _VP], "alz_plan_destroy_multi": [_VP],
    "alz_encode_batch": [_VP, _VP, _VP, _U32, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP],
    "alz_encode_batch_device": [_VP, _VP, _VP, _U32, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP],
    "alz_encode_batch_multi": [_VPP, _U32, _VP, _VP, _U32, _VP, _SZ, _VP, _VP, _SZ, _VP, _VP, _VP],
    "alz_device_malloc": [_VP, _SZ, _VPP], "alz_device_free": [_VP, _VP],
    "alz_memcpy_h2d": [_VP, _VP, _VP, _SZ], "alz_memcpy_d2h": [_VP, _VP, _VP, _SZ], "alz_memset_d": [_VP, _VP, C.c_int, _SZ],
    "alz_synchronize": [_VP],
    "alz_measure_copy_bandwidth": [_VP, _SZ, C.c_int, C.POINTER(C.c_double)], "alz_last_kernel_ms": [_VP, C.POINTER(C.c_float)],
}
CORE_RESTYPES = {"alz_last_error": C.c_char_p, "alz_destroy": None, "alz_plan_destroy": None, "alz_plan_destroy_multi": None}

# the container layer: a whole file of one alz_container in host memory (alz_container_measure is with the measure entry points)
CONTAINER_PROTOTYPES = {
    "alz_container_is_match": [_U32, _VP, _SZ],
    "alz_container_decompressed_size": [_U32, _VP, _VP, _SZ, _U32P],
    "alz_container_decompress": [_VP, _U32, _VP, _VP, _SZ, _VP, _SZ, _SZP, _SZP, _I32P],
    "alz_container_compress": [_VP, _U32, _VP, _VP, _VP, _SZ, _VP, _SZ, _SZP],
    "alz_container_compress_bound": [_U32, _SZ],                                   # returns size_t (CONTAINER_RESTYPES)
}
CONTAINER_RESTYPES = {"alz_container_compress_bound": C.c_size_t}

# the batch producers of the reference's CLI (scan.py)
SCAN_PROTOTYPES = {
    "alz_container_scan": [_VP, _VP, _U32, _VP, _VP, _SZ, _VP, _SZ, _VP, _U32, _U32P, _SZP],
    "alz_brute_decoder_name": [_U32],                                              # returns const char*
    "alz_brute_force": [_VP, _VP, _SZ, _U32, _VP, _SZ, _VP],
}
SCAN_RESTYPES = {"alz_brute_decoder_name": C.c_char_p}

# the measure entry points (include/auroralz.h): decoded sizes without decoding
MEASURE_NO_BOUND = 0xFFFFFF00          # the largest dst_cap: "count everything"
MEASURE_PROTOTYPES = {
    "alz_measure_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    "alz_measure_batch_device": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
    "alz_container_measure": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)],
}

# the RLE30 / HUF20 entry points: (ctx, n, src_base, src_bytes, streams, dst_base, dst_bytes, results)
RLH_PROTOTYPES = {name: [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
                  for name in ("alz_rlh_decode_batch", "alz_rlh_decode_batch_device", "alz_rlh_encode_batch", "alz_rlh_encode_batch_device")}

# the RLHudson entry points (RLE30's sibling, a family with one kind): the same parameter list; `format`, aux0 and aux1 of a stream are ignored
RLHUDSON_PROTOTYPES = {name: RLH_PROTOTYPES["alz_rlh_decode_batch"]
                       for name in ("alz_rlhudson_decode_batch", "alz_rlhudson_decode_batch_device", "alz_rlhudson_encode_batch", "alz_rlhudson_encode_batch_device")}
RLHUDSON_PROTOTYPES["alz_rlhudson_encode_bound"] = [C.c_size_t]
RLHUDSON_RESTYPES = {"alz_rlhudson_encode_bound": C.c_size_t}

# the aPLib entry points (decode only): batches of headerless bodies, their sizes without decoding, and the aPLib class on a file in host memory
APLIB_WINDOW = 0x200000
_APLIB_DECODE = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
_APLIB_MEASURE = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
APLIB_PROTOTYPES = {
    "alz_aplib_decode_batch": _APLIB_DECODE, "alz_aplib_decode_batch_device": _APLIB_DECODE,
    "alz_aplib_measure_batch": _APLIB_MEASURE, "alz_aplib_measure_batch_device": _APLIB_MEASURE,
    "alz_aplib_is_match": [C.c_void_p, C.c_size_t],
    "alz_aplib_decompressed_size": [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)],
    "alz_aplib_decompress": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)],
}

# the CRILAYLA / ALLZ entry points (decode only): batches of headerless bodies (streams[i].format is a BITLZ_* value) and the two classes on a file in host memory
BITLZ_CRILAYLA, BITLZ_ALLZ = range(2)
BITLZ_COUNT = 2
BITLZ_NAMES = ["crilayla", "allz"]
CRILAYLA_HEADER = 0x100                 # plain bytes a CRILAYLA file keeps behind its body; the file layer decodes into size + 0x100
CRILAYLA_MAX_DISTANCE = 8194


def allz_aux0(copy_bits=0, dist_bits=10, len_bits=1):
    """ALZ_ALLZ_AUX0: flags[1], flags[2], flags[3] of an ALLZ header (the class defaults)."""
    return copy_bits | dist_bits << 8 | len_bits << 16


_BITLZ_DECODE = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
_BITLZ_IS_MATCH = [C.c_void_p, C.c_size_t]
_BITLZ_SIZE = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
_BITLZ_DECOMPRESS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
BITLZ_PROTOTYPES = {
    "alz_bitlz_decode_batch": _BITLZ_DECODE, "alz_bitlz_decode_batch_device": _BITLZ_DECODE,
    "alz_crilayla_is_match": _BITLZ_IS_MATCH, "alz_crilayla_decompressed_size": _BITLZ_SIZE, "alz_crilayla_decompress": _BITLZ_DECOMPRESS,
    "alz_allz_is_match": _BITLZ_IS_MATCH, "alz_allz_decompressed_size": _BITLZ_SIZE, "alz_allz_decompress": _BITLZ_DECOMPRESS,
}

# CRILAYLA / ALLZ written (CompressHeaderless of the two classes): batches of raw buffers (streams[i].format a BITLZ_* value, an ALLZ stream's aux0 = allz_aux0(...))
# and the two classes' files; settings is an alz_settings* (NULL: quality 8)
_BITENC_ENCODE = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
BITENC_PROTOTYPES = {
    "alz_bitenc_bound": [C.c_uint32, C.c_size_t],                                  # returns size_t (BITENC_RESTYPES)
    "alz_bitenc_encode_batch": _BITENC_ENCODE, "alz_bitenc_encode_batch_device": _BITENC_ENCODE,
    "alz_bitenc_file_bound": [C.c_uint32, C.c_size_t],                             # returns size_t
    "alz_bitenc_file_compress": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "alz_bitenc_file_compress_batch": _BITENC_ENCODE,
}
BITENC_RESTYPES = {"alz_bitenc_bound": C.c_size_t, "alz_bitenc_file_bound": C.c_size_t}

# aPLib written (aPLib.CompressHeaderless / Compress): batches of raw buffers (format, aux0, aux1 and decom_len of a stream are ignored) and "AP32" files;
# settings is an alz_settings* (NULL: quality 8)
APENC_PROTOTYPES = {
    "alz_apenc_bound": [C.c_size_t],                                               # returns size_t (APENC_RESTYPES)
    "alz_apenc_encode_batch": _BITENC_ENCODE, "alz_apenc_encode_batch_device": _BITENC_ENCODE,
    "alz_apenc_file_bound": [C.c_size_t],                                          # returns size_t
    "alz_apenc_file_compress": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "alz_apenc_file_compress_batch": _BITENC_ENCODE,
}
APENC_RESTYPES = {"alz_apenc_bound": C.c_size_t, "alz_apenc_file_bound": C.c_size_t}

# the DEFLATE entry points (decode only): batches of raw streams, their sizes without decoding, and the ZLib / GZip classes on a file in host memory
INFLATE_WINDOW = 0x8000
_INFLATE_DECODE = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
_INFLATE_MEASURE = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
_INFLATE_IS_MATCH = [C.c_void_p, C.c_size_t]
_INFLATE_DECOMPRESS = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
_INFLATE_FILE_MEASURE = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
INFLATE_PROTOTYPES = {
    "alz_inflate_decode_batch": _INFLATE_DECODE, "alz_inflate_decode_batch_device": _INFLATE_DECODE,
    "alz_inflate_measure_batch": _INFLATE_MEASURE, "alz_inflate_measure_batch_device": _INFLATE_MEASURE,
    "alz_zlib_is_match": _INFLATE_IS_MATCH, "alz_gzip_is_match": _INFLATE_IS_MATCH,
    "alz_zlib_decompress": _INFLATE_DECOMPRESS, "alz_gzip_decompress": _INFLATE_DECOMPRESS,
    "alz_zlib_measure": _INFLATE_FILE_MEASURE, "alz_gzip_measure": _INFLATE_FILE_MEASURE,
}

# checksums of byte ranges on the GPU (a range is src_off / src_len of a Stream) and the host arithmetic that joins two of them
CK_ADLER32 = 0
CK_CRC32 = 1
_CHECKSUM_BATCH = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
CHECKSUM_PROTOTYPES = {
    "alz_checksum_batch": _CHECKSUM_BATCH, "alz_checksum_batch_device": _CHECKSUM_BATCH,
    "alz_checksum_combine": [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64],      # returns uint32_t (CHECKSUM_RESTYPES)
}
CHECKSUM_RESTYPES = {"alz_checksum_combine": C.c_uint32}

# ZLib and GZip files in batches: Stream.format selects the class, one FileResult per file
ZFILE_ZLIB = 0
ZFILE_GZIP = 1


class FileResult(C.Structure):
    """alz_file_result: what the single-file call returns for the file -- its rc, the alz_status, bytes delivered, source bytes used"""
    _fields_ = [("rc", C.c_int32), ("status", C.c_int32), ("dst_len", C.c_uint32), ("src_used", C.c_uint32)]


ZFILE_PROTOTYPES = {
    "alz_zfile_decode_batch": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "alz_zfile_measure_batch": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
}

# XXH32 of byte ranges on the GPU: the checksum family's argument list with a seed in place of the kind
_XXH32_BATCH = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
XXH32_PROTOTYPES = {"alz_xxh32_batch": _XXH32_BATCH, "alz_xxh32_batch_device": _XXH32_BATCH}

# LZ4 (frame, legacy) and framed Snappy files in batches: Stream.format is C_LZ4_FRAME, C_LZ4_LEGACY or C_SNAPPY, one FileResult per file
FRAMED_CONTAINERS = (C_LZ4_FRAME, C_LZ4_LEGACY, C_SNAPPY)
FRAMED_PROTOTYPES = {
    "alz_framed_decode_batch": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "alz_framed_measure_batch": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p],
}

# CRC-32C of byte ranges on the GPU (the checksum of a framed Snappy chunk, before its mask): the checksum family's argument list without a kind
_CRC32C_BATCH = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32)]
CRC32C_PROTOTYPES = {
    "alz_crc32c_batch": _CRC32C_BATCH, "alz_crc32c_batch_device": _CRC32C_BATCH,
    "alz_crc32c_combine": [C.c_uint32, C.c_uint32, C.c_uint64],                    # returns uint32_t (CRC32C_RESTYPES)
}
CRC32C_RESTYPES = {"alz_crc32c_combine": C.c_uint32}

# LZ4 (frame, legacy) and framed Snappy files WRITTEN in batches: Stream.format is one of FRAMED_CONTAINERS, aux0 an LZ4 frame's block size
FRAMING_COMPRESS_PROTOTYPES = {
    "alz_framing_compress_batch": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
}

# the wrapped files (alz_wfile_*): RLHudson and the seven wrapper classes of the .Extended assembly; in a batch Stream.format is the kind, aux0 bit 0 the byte order
WF_ASURAZLB, WF_ZLB, WF_MDF0, WF_RAREZIP, WF_HWGZ, WF_SSZL, WF_ZLWF, WF_RLHUDSON = range(8)
WF_COUNT = 8
WF_NAMES = ["asurazlb", "zlb", "mdf0", "rarezip", "hwgz", "sszl", "zlwf", "rlhudson"]
WB_ZLIB, WB_GZIP, WB_DEFLATE, WB_WFLZ, WB_WFLZ_BE, WB_RLHUDSON, WB_PLAIN = range(7)
SSZL_COMPRESSED, SSZL_USE_GZIP, SSZL_ENCRYPTED = 0x1, 0x2, 0x80000000


class WfilePart(C.Structure):
    """alz_wfile_part"""
    _fields_ = [("src_off", C.c_uint32), ("src_len", C.c_uint32), ("body", C.c_uint32), ("dst_len", C.c_uint32)]


WFILE_PROTOTYPES = {
    "alz_wfile_is_match": [C.c_uint32, C.c_void_p, C.c_size_t],
    "alz_wfile_decompressed_size": [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, _U32P],
    "alz_wfile_walk": [C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, _U32P, _U32P, _U32P],
    "alz_wfile_decompress": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _SZP, _SZP, C.POINTER(C.c_int32)],
    "alz_wfile_decode_batch": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p],
    "alz_wfile_compress_bound": [C.c_uint32, C.c_void_p, C.c_size_t],
    "alz_wfile_compress": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, _SZP],
}
WFILE_RESTYPES = {"alz_wfile_compress_bound": C.c_size_t}

# DEFLATE written on the GPU: raw streams (level 0..9, flags DEFLATE_FIXED) and ZLib / GZip files (kind: ZFILE_ZLIB / ZFILE_GZIP, in a batch Stream.format)
DEFLATE_FIXED = 1
_DEFLATE_ENCODE = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
DEFLATE_PROTOTYPES = {
    "alz_deflate_bound": [C.c_size_t],                                            # returns size_t (DEFLATE_RESTYPES)
    "alz_deflate_block_bytes": [],
    "alz_deflate_encode_batch": _DEFLATE_ENCODE, "alz_deflate_encode_batch_device": _DEFLATE_ENCODE,
    "alz_deflate_file_bound": [C.c_uint32, C.c_size_t],                           # returns size_t
    "alz_deflate_file_compress": [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)],
    "alz_deflate_file_compress_batch": _DEFLATE_ENCODE,
}
DEFLATE_RESTYPES = {"alz_deflate_bound": C.c_size_t, "alz_deflate_file_bound": C.c_size_t}

# all of them: what _lib.load() sets on the loaded library
PROTOTYPES = {name: types for table, rows in list(globals().items()) if table.endswith("_PROTOTYPES") for name, types in rows.items()}
RESTYPES = {name: t for table, rows in list(globals().items()) if table.endswith("_RESTYPES") for name, t in rows.items()}

assert C.sizeof(Stream) == 40 and C.sizeof(Result) == 16 and C.sizeof(LzProperties) == 16 and C.sizeof(FileResult) == 16
