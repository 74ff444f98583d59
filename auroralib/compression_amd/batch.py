"""Thin object layer over the batch half of the C ABI (context, plans, device buffers)."""
import ctypes as C

import numpy as np

from . import _abi as A
from . import _lib as _libmod
from ._lib import check, load


def _vp(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    return a


def _ref(lz):
    return C.byref(lz) if lz is not None else None


def _settings(quality, strategy=0, min_distance=0, max_window_bits=0):
    """the alz_settings* of a call"""
    return C.byref(A.Settings(quality, max_window_bits, strategy, min_distance))


def _encode_aux(streams):
    """one alz_encode_aux per stream: the trailing array of the alz_encode_batch* calls"""
    return (A.EncodeAux * len(streams))()


def _dst_array(dst, dst_bytes):
    """the destination of a host-buffer call: a new zeroed array, or the caller's own after a check of its shape"""
    if dst is None:
        return np.zeros(max(dst_bytes, 1), dtype=np.uint8)
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or dst.nbytes < dst_bytes:
        raise ValueError("dst must be a contiguous uint8 array of at least dst_bytes")
    return dst


def device_count():
    """alz_device_count: HIP devices visible to this process (0 without a GPU)."""
    _libmod.GPU_TOUCHED = True
    return int(load().alz_device_count())


class Context:
    """alz_ctx: one HIP device + one HIP stream."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        _libmod.GPU_TOUCHED = True
        check(self.lib.alz_create(device, C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.alz_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_uint64()
        check(self.lib.alz_device_info(self.h, name, 256, C.byref(cu), C.byref(mem)))
        return {"name": name.value.decode(), "cu_count": cu.value, "hbm_bytes": mem.value}

    def set_exact_kernels(self, on):
        """Kernel family of this context: the exact one-token-at-a-time kernels instead of the lane-parallel ones."""
        check(self.lib.alz_ctx_set_exact_kernels(self.h, 1 if on else 0))

    def set_kernel_variant(self, variant):
        """alz_ctx_set_kernel_variant: 0 the library chooses, 1 / 2 one / two wavefronts per stream where both shapes exist."""
        check(self.lib.alz_ctx_set_kernel_variant(self.h, variant))

    def big_stream(self, min_bytes=0):
        """alz_ctx_big_stream: threshold of the whole-GPU paths for ONE stream of the north-star bodies -- decode from `min_bytes` of output on
        (default 24 KiB), encode from min(min_bytes, 8 KiB) of input on; 0 keeps the current value, 0xFFFFFFFF switches both paths off.
        Returns how many streams have taken either path on this context."""
        n = C.c_uint64()
        check(self.lib.alz_ctx_big_stream(self.h, min_bytes, C.byref(n)))
        return n.value

    def release_scratch(self):
        """alz_ctx_release_scratch: return the grow-only staging / encoder scratch of the host-buffer calls to the device."""
        check(self.lib.alz_ctx_release_scratch(self.h))

    def copy_bandwidth(self, nbytes=1 << 30, iters=10):
        """Measured device-to-device copy bandwidth in GB/s (bytes read + written): the second roofline denominator."""
        v = C.c_double()
        check(self.lib.alz_measure_copy_bandwidth(self.h, nbytes, iters, C.byref(v)))
        return v.value

    def last_kernel_ms(self):
        v = C.c_float()
        check(self.lib.alz_last_kernel_ms(self.h, C.byref(v)))
        return v.value

    # ---- the shapes of a batch call.  `lead`: what the C function takes between the context and n (alz_lz_properties, alz_settings, a level, nothing);
    # files: the table is one of whole files, answered by one alz_file_result per file; aux: arrays the C function takes behind the results
    def _host_decode(self, fn, lead, streams, src, dst_bytes, dst=None, files=False, aux=()):
        """fn(ctx, *lead, n, src, src_bytes, streams, dst, dst_bytes, results, *aux) on host buffers -> (dst, results)"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        dst = _dst_array(dst, dst_bytes)
        return dst, self._device(fn, lead, streams, _vp(src), src.nbytes, _vp(dst), dst_bytes, files=files, aux=aux)

    def _host_measure(self, fn, lead, streams, src, files=False):
        """fn(ctx, *lead, n, src, src_bytes, streams, results) on a host buffer -> results"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        return self._device(fn, lead, streams, _vp(src), src.nbytes, files=files)

    def _device(self, fn, lead, streams, d_src, src_bytes, *dst, files=False, aux=()):
        """fn(ctx, *lead, n, d_src, src_bytes, streams, [d_dst, dst_bytes,] results, *aux) -> results"""
        res = (A.FileResult * len(streams))() if files else (A.Result * len(streams))()
        check(fn(self.h, *lead, len(streams), d_src, src_bytes, streams, *dst, res, *aux))
        return res

    def _host_ranges(self, fn, lead, ranges, src):
        """fn(ctx, *lead, n, src, src_bytes, ranges, uint32[]) on a host buffer -> one uint32 per range"""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        return self._ranges(fn, lead, ranges, _vp(src), src.nbytes)

    def _ranges(self, fn, lead, ranges, d_src, src_bytes):
        """fn(ctx, *lead, n, d_src, src_bytes, ranges, uint32[]) -> one uint32 per range"""
        out = np.zeros(max(len(ranges), 1), dtype=np.uint32)
        check(fn(self.h, *lead, len(ranges), d_src, src_bytes, ranges, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:len(ranges)]

    # ---- host-buffer decode (upload, decode on GPU, download)
    def decode_batch(self, streams, src, dst_bytes, lz=None, dst=None):
        """alz_decode_batch on host buffers.  `dst`: a caller-owned uint8 array of >= dst_bytes to decode into (default: a new one)."""
        return self._host_decode(self.lib.alz_decode_batch, (_ref(lz),), streams, src, dst_bytes, dst)

    def decode(self, fmt, src, decom_len=0, cap=None, aux0=0, aux1=0, lz=None):
        src = bytes(src)
        cap = decom_len if cap is None else cap
        dst = np.empty(max(cap, 1), dtype=np.uint8)          # (untouched memory: a ctypes buffer would be written full of zeros first)
        r = A.Result()
        check(self.lib.alz_decode(self.h, fmt, _ref(lz), src, len(src), decom_len, aux0, aux1, _vp(dst), cap, C.byref(r)))
        return dst[:r.dst_len].tobytes(), r

    # ---- decoded sizes without decoding
    def measure_batch(self, streams, src, lz=None):
        """alz_measure_batch on a host buffer: the results alz_decode_batch would return for `streams` (status, dst_len, src_used), nothing decoded.
        dst_off is ignored and dst_cap only bounds the count (A.MEASURE_NO_BOUND: the true size)."""
        return self._host_measure(self.lib.alz_measure_batch, (_ref(lz),), streams, src)

    def measure_batch_device(self, streams, d_src, src_bytes, lz=None):
        """alz_measure_batch_device: the same with the source already in HBM at d_src; last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_measure_batch_device, (_ref(lz),), streams, d_src, src_bytes)

    # ---- RLE30 / HUF20: the non-LZ bodies of the GBA / DS family (streams[i].format is an A.RLH_* value)
    def rlh_decode_batch(self, streams, src, dst_bytes):
        """alz_rlh_decode_batch on host buffers: RLE30 / HUF20 bodies; aux0 of a HUF20_4 stream is the nibble order (1 = big, Level5)."""
        return self._host_decode(self.lib.alz_rlh_decode_batch, (), streams, src, dst_bytes)

    def rlh_encode_batch(self, streams, src, dst_bytes):
        """alz_rlh_encode_batch: RLE30.CompressHeaderless of raw buffers (a HUF format raises AlzError E_UNSUPPORTED: there is no encoder)."""
        return self._host_decode(self.lib.alz_rlh_encode_batch, (), streams, src, dst_bytes)

    def rlh_decode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_rlh_decode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_rlh_decode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    def rlh_encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_rlh_encode_batch_device: raw buffers in HBM at d_src, RLE30 streams left at d_dst."""
        return self._device(self.lib.alz_rlh_encode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    # ---- RLHudson: RLE30's sibling, a family with one kind (format, aux0 and aux1 of a stream are ignored)
    def rlhudson_decode_batch(self, streams, src, dst_bytes):
        """alz_rlhudson_decode_batch on host buffers: headerless RLHudson bodies, decom_len is the size their header states."""
        return self._host_decode(self.lib.alz_rlhudson_decode_batch, (), streams, src, dst_bytes)

    def rlhudson_encode_batch(self, streams, src, dst_bytes):
        """alz_rlhudson_encode_batch: RLHudson.CompressHeaderless of raw buffers, bit-identical to the managed bytes (alz_rlhudson_encode_bound per buffer suffices)."""
        return self._host_decode(self.lib.alz_rlhudson_encode_batch, (), streams, src, dst_bytes)

    def rlhudson_decode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_rlhudson_decode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launch."""
        return self._device(self.lib.alz_rlhudson_decode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    def rlhudson_encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_rlhudson_encode_batch_device: raw buffers in HBM at d_src, RLHudson bodies left at d_dst."""
        return self._device(self.lib.alz_rlhudson_encode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    # ---- aPLib (decode only): headerless bodies; format, decom_len, aux0 and aux1 of a stream are ignored
    def aplib_decode_batch(self, streams, src, dst_bytes, dst=None):
        """alz_aplib_decode_batch on host buffers.  `dst`: a caller-owned uint8 array of >= dst_bytes to decode into (default: a new one)."""
        return self._host_decode(self.lib.alz_aplib_decode_batch, (), streams, src, dst_bytes, dst)

    def aplib_decode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_aplib_decode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launch."""
        return self._device(self.lib.alz_aplib_decode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    def aplib_measure_batch(self, streams, src):
        """alz_aplib_measure_batch on a host buffer: the results aplib_decode_batch would return, nothing decoded; dst_cap only bounds the count."""
        return self._host_measure(self.lib.alz_aplib_measure_batch, (), streams, src)

    def aplib_measure_batch_device(self, streams, d_src, src_bytes):
        """alz_aplib_measure_batch_device: the same with the source already in HBM at d_src."""
        return self._device(self.lib.alz_aplib_measure_batch_device, (), streams, d_src, src_bytes)

    # ---- CRILAYLA / ALLZ (decode only): headerless bodies; streams[i].format is an A.BITLZ_* value
    def bitlz_decode_batch(self, streams, src, dst_bytes, dst=None):
        """alz_bitlz_decode_batch on host buffers.  A CRILAYLA stream's dst_len bytes end at dst_off + dst_cap (it is written from the top down);
        an ALLZ stream takes decom_len and aux0 = A.allz_aux0(copy, dist, len).  `dst`: a caller-owned uint8 array of >= dst_bytes (default: a new one)."""
        return self._host_decode(self.lib.alz_bitlz_decode_batch, (), streams, src, dst_bytes, dst)

    def bitlz_decode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_bitlz_decode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_bitlz_decode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    # ---- CRILAYLA / ALLZ written: raw buffers in (src_*), headerless bodies out (dst_*); streams[i].format is an A.BITLZ_* value
    def bitenc_encode_batch(self, streams, src, dst_bytes, quality=8, strategy=0, dst=None):
        """alz_bitenc_encode_batch on host buffers -> (dst, results): CompressHeaderless of the two classes, the managed bytes for the same settings.
        A body occupies [dst_off, dst_off + dst_len); an ALLZ stream takes aux0 = A.allz_aux0(copy, dist, len).  ALLZ at quality 1 raises AlzError
        E_UNSUPPORTED.  A lone large buffer goes through the same batch pipeline as many small ones."""
        return self._host_decode(self.lib.alz_bitenc_encode_batch, (_settings(quality, strategy),), streams, src, dst_bytes, dst)

    def bitenc_encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes, quality=8, strategy=0):
        """alz_bitenc_encode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_bitenc_encode_batch_device, (_settings(quality, strategy),), streams, d_src, src_bytes, d_dst, dst_bytes)

    def bitenc_file_compress_batch(self, files, src, dst_bytes, quality=8, strategy=0, dst=None):
        """alz_bitenc_file_compress_batch on host buffers -> (dst, results): per file (Stream.format an A.BITLZ_* value, aux0 ALLZ's start bits) what
        alz_bitenc_file_compress writes and returns for it alone; all bodies are one encode batch."""
        return self._host_decode(self.lib.alz_bitenc_file_compress_batch, (_settings(quality, strategy),), files, src, dst_bytes, dst, files=True)

    # ---- aPLib written: raw buffers in (src_*), headerless bodies out (dst_*); format, aux0, aux1 and decom_len of a stream are ignored
    def apenc_encode_batch(self, streams, src, dst_bytes, quality=8, strategy=0, dst=None):
        """alz_apenc_encode_batch on host buffers -> (dst, results): aPLib.CompressHeaderless, the managed bytes for the same settings.  A body
        occupies [dst_off, dst_off + dst_len).  An empty stream raises AlzError E_INVALID; at qualities 1..7 a stream longer than the managed
        chain table (2^18 / 2^19 / 2^20 bytes) raises E_UNSUPPORTED.  A lone large buffer goes through the same batch pipeline as many small ones."""
        return self._host_decode(self.lib.alz_apenc_encode_batch, (_settings(quality, strategy),), streams, src, dst_bytes, dst)

    def apenc_encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes, quality=8, strategy=0):
        """alz_apenc_encode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_apenc_encode_batch_device, (_settings(quality, strategy),), streams, d_src, src_bytes, d_dst, dst_bytes)

    def apenc_file_compress_batch(self, files, src, dst_bytes, quality=8, strategy=0, dst=None):
        """alz_apenc_file_compress_batch on host buffers -> (dst, results): per file what alz_apenc_file_compress writes and returns for it
        alone ("AP32", the 24-byte header, the body); all bodies are one encode batch."""
        return self._host_decode(self.lib.alz_apenc_file_compress_batch, (_settings(quality, strategy),), files, src, dst_bytes, dst, files=True)

    # ---- DEFLATE (decode only): raw streams as zlib's inflate reads them; format, decom_len, aux0 and aux1 of a stream are ignored
    def inflate_decode_batch(self, streams, src, dst_bytes, dst=None):
        """alz_inflate_decode_batch on host buffers.  `dst`: a caller-owned uint8 array of >= dst_bytes to decode into (default: a new one)."""
        return self._host_decode(self.lib.alz_inflate_decode_batch, (), streams, src, dst_bytes, dst)

    def inflate_decode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes):
        """alz_inflate_decode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launch."""
        return self._device(self.lib.alz_inflate_decode_batch_device, (), streams, d_src, src_bytes, d_dst, dst_bytes)

    def inflate_measure_batch(self, streams, src):
        """alz_inflate_measure_batch on a host buffer: the results inflate_decode_batch would return, nothing decoded; dst_cap only bounds the count."""
        return self._host_measure(self.lib.alz_inflate_measure_batch, (), streams, src)

    def inflate_measure_batch_device(self, streams, d_src, src_bytes):
        """alz_inflate_measure_batch_device: the same with the source already in HBM at d_src."""
        return self._device(self.lib.alz_inflate_measure_batch_device, (), streams, d_src, src_bytes)

    # ---- checksums of byte ranges: kind is A.CK_ADLER32 or A.CK_CRC32; a range is src_off / src_len of its Stream
    def _checksum(self, fn, kind, ranges, d_src, src_bytes):
        """either form of the call on a source that is already a pointer (tests/test_gpu_checksum.py holds the two forms against each other this way)"""
        return self._ranges(fn, (kind,), ranges, d_src, src_bytes)

    def checksum_batch(self, kind, ranges, src):
        """alz_checksum_batch on a host buffer -> a uint32 array, one checksum per range."""
        return self._host_ranges(self.lib.alz_checksum_batch, (kind,), ranges, src)

    def checksum_batch_device(self, kind, ranges, d_src, src_bytes):
        """alz_checksum_batch_device: the same with the bytes already in HBM at d_src; last_kernel_ms() is the device time of the two launches."""
        return self._checksum(self.lib.alz_checksum_batch_device, kind, ranges, d_src, src_bytes)

    # ---- ZLib and GZip files in batches: Stream.format is A.ZFILE_ZLIB or A.ZFILE_GZIP, src_off / src_len the whole file
    def zfile_decode_batch(self, files, src, dst_bytes, dst=None):
        """alz_zfile_decode_batch on host buffers -> (dst, results): per file what alz_zlib_decompress / alz_gzip_decompress return for it alone.
        `dst`: a caller-owned uint8 array of >= dst_bytes to decode into (default: a new one)."""
        return self._host_decode(self.lib.alz_zfile_decode_batch, (), files, src, dst_bytes, dst, files=True)

    def wfile_decode_batch(self, files, src, dst_bytes, dst=None):
        """alz_wfile_decode_batch on host buffers -> (dst, results): files[i].format is an A.WF_* kind (a batch may mix them), aux0 bit 0 the byte
        order of an HWGZ / ZLWF file; per file what alz_wfile_decompress returns for it alone."""
        return self._host_decode(self.lib.alz_wfile_decode_batch, (), files, src, dst_bytes, dst, files=True)

    def zfile_measure_batch(self, files, src):
        """alz_zfile_measure_batch on a host buffer -> results: per file what alz_zlib_measure / alz_gzip_measure return; dst_cap is the size limit."""
        return self._host_measure(self.lib.alz_zfile_measure_batch, (), files, src, files=True)

    # ---- XXH32 of byte ranges (the checksum of the LZ4 frame format); a range is src_off / src_len of its Stream
    def xxh32_batch(self, ranges, src, seed=0):
        """alz_xxh32_batch on a host buffer -> a uint32 array, one XXH32 per range."""
        return self._host_ranges(self.lib.alz_xxh32_batch, (seed,), ranges, src)

    def xxh32_batch_device(self, ranges, d_src, src_bytes, seed=0):
        """alz_xxh32_batch_device: the same with the bytes already in HBM at d_src; last_kernel_ms() is the device time of the launch."""
        return self._ranges(self.lib.alz_xxh32_batch_device, (seed,), ranges, d_src, src_bytes)

    # ---- LZ4 and Snappy files in batches: Stream.format is A.C_LZ4_FRAME, A.C_LZ4_LEGACY or A.C_SNAPPY, src_off / src_len the whole file
    def framed_decode_batch(self, files, src, dst_bytes, dst=None):
        """alz_framed_decode_batch on host buffers -> (dst, results): per file what alz_container_decompress returns for it alone.
        `dst`: a caller-owned uint8 array of >= dst_bytes to decode into (default: a new one)."""
        return self._host_decode(self.lib.alz_framed_decode_batch, (), files, src, dst_bytes, dst, files=True)

    def framed_measure_batch(self, files, src):
        """alz_framed_measure_batch on a host buffer -> results: per file what alz_container_measure returns; dst_cap is the size limit."""
        return self._host_measure(self.lib.alz_framed_measure_batch, (), files, src, files=True)

    # ---- CRC-32C of byte ranges (the checksum of a framed Snappy chunk, before its mask); a range is src_off / src_len of its Stream
    def crc32c_batch(self, ranges, src):
        """alz_crc32c_batch on a host buffer -> a uint32 array, one CRC-32C per range."""
        return self._host_ranges(self.lib.alz_crc32c_batch, (), ranges, src)

    def crc32c_batch_device(self, ranges, d_src, src_bytes):
        """alz_crc32c_batch_device: the same with the bytes already in HBM at d_src; last_kernel_ms() is the device time of the two launches."""
        return self._ranges(self.lib.alz_crc32c_batch_device, (), ranges, d_src, src_bytes)

    # ---- LZ4 and Snappy files written in batches: Stream.format is A.C_LZ4_FRAME, A.C_LZ4_LEGACY or A.C_SNAPPY, src_off / src_len the raw input
    def framing_compress_batch(self, files, src, dst_bytes, dst=None, quality=8, strategy=0, min_distance=0, max_window_bits=0):
        """alz_framing_compress_batch on host buffers -> (dst, results): per file what alz_container_compress writes and returns for it alone
        (aux0: the block size of an LZ4 frame).  `dst`: a caller-owned uint8 array of >= dst_bytes to write into (default: a new one)."""
        st = _settings(quality, strategy, min_distance, max_window_bits)
        return self._host_decode(self.lib.alz_framing_compress_batch, (st,), files, src, dst_bytes, dst, files=True)

    # ---- DEFLATE written on the GPU: raw streams (src_* the raw input, dst_* where the stream goes); level 0..9, flags A.DEFLATE_FIXED
    def deflate_encode_batch(self, streams, src, dst_bytes, level=6, flags=0, dst=None):
        """alz_deflate_encode_batch on host buffers -> (dst, results).  `dst`: a caller-owned uint8 array of >= dst_bytes to write into (default: a new one)."""
        return self._host_decode(self.lib.alz_deflate_encode_batch, (level, flags), streams, src, dst_bytes, dst)

    def deflate_encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes, level=6, flags=0):
        """alz_deflate_encode_batch_device: both buffers in HBM; returns the results, last_kernel_ms() is the device time of the launches."""
        return self._device(self.lib.alz_deflate_encode_batch_device, (level, flags), streams, d_src, src_bytes, d_dst, dst_bytes)

    def deflate_file_compress_batch(self, files, src, dst_bytes, level=6, flags=0, dst=None):
        """alz_deflate_file_compress_batch on host buffers -> (dst, results): per file (Stream.format: A.ZFILE_ZLIB or A.ZFILE_GZIP) what
        alz_deflate_file_compress writes and returns for it alone.  `dst`: a caller-owned uint8 array of >= dst_bytes (default: a new one)."""
        return self._host_decode(self.lib.alz_deflate_file_compress_batch, (level, flags), files, src, dst_bytes, dst, files=True)

    # ---- host-buffer encode
    def encode_batch(self, streams, src, dst_bytes, quality=8, lz=None, strategy=0, min_distance=0, max_window_bits=0):
        """alz_encode_batch: streams describe RAW inputs (src_*) and compressed-output capacity (dst_*)."""
        st, aux = _settings(quality, strategy, min_distance, max_window_bits), _encode_aux(streams)
        dst, res = self._host_decode(self.lib.alz_encode_batch, (_ref(lz), st), streams, src, dst_bytes, aux=(aux,))
        return dst, res, aux

    def encode_batch_device(self, streams, d_src, src_bytes, d_dst, dst_bytes, quality=8, lz=None, strategy=0, min_distance=0, max_window_bits=0):
        """alz_encode_batch_device: raw buffers already in HBM at d_src, compressed streams left in HBM at d_dst (offsets of
        `streams` are relative to the two device pointers).  Returns (results, aux); last_kernel_ms() is the device time."""
        st, aux = _settings(quality, strategy, min_distance, max_window_bits), _encode_aux(streams)
        return self._device(self.lib.alz_encode_batch_device, (_ref(lz), st), streams, d_src, src_bytes, d_dst, dst_bytes, aux=(aux,)), aux

    # ---- device memory
    def malloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.alz_device_malloc(self.h, nbytes, C.byref(p)))
        return p

    def free(self, p):
        check(self.lib.alz_device_free(self.h, p))

    def h2d(self, d, arr):
        arr = np.ascontiguousarray(arr)
        check(self.lib.alz_memcpy_h2d(self.h, d, _vp(arr), arr.nbytes))

    def d2h(self, d, nbytes, offset=0):
        out = np.empty(nbytes, dtype=np.uint8)
        check(self.lib.alz_memcpy_d2h(self.h, _vp(out), C.c_void_p(d.value + offset), nbytes))
        return out

    def memset(self, d, value, nbytes):
        check(self.lib.alz_memset_d(self.h, d, value, nbytes))

    def synchronize(self):
        check(self.lib.alz_synchronize(self.h))


class Plan:
    """alz_plan: descriptor table resident in HBM, grouped per format."""

    def __init__(self, ctx, streams, lz=None):
        self.ctx, self.n = ctx, len(streams)
        h = C.c_void_p()
        check(ctx.lib.alz_plan_create(ctx.h, _ref(lz), self.n, streams, C.byref(h)))
        self.h = h

    def execute(self, d_src, d_dst, hip_stream=None):
        check(self.ctx.lib.alz_plan_execute(self.ctx.h, self.h, d_src, d_dst, hip_stream))

    def execute_timed(self, d_src, d_dst, iters=1):
        ms = C.c_float()
        check(self.ctx.lib.alz_plan_execute_timed(self.ctx.h, self.h, d_src, d_dst, iters, C.byref(ms)))
        return ms.value

    def results(self):
        res = (A.Result * self.n)()
        check(self.ctx.lib.alz_plan_results(self.ctx.h, self.h, res))
        return res

    def close(self):
        if self.h:
            self.ctx.lib.alz_plan_destroy(self.ctx.h, self.h)
            self.h = None


class MultiPlan:
    """alz_multi_plan: ONE device-resident batch over several contexts (one per GPU) -- the batch partitioned by the library (or by `part_of`),
    one plan per context, no host staging, no collective.  A stream's offsets are relative to the device buffers of ITS context."""

    def __init__(self, ctxs, streams, lz=None, part_of=None):
        self.ctxs, self.n = list(ctxs), len(streams)
        self.lib = self.ctxs[0].lib
        arr = (C.c_void_p * len(self.ctxs))(*[c.h for c in self.ctxs])
        part = np.zeros(max(self.n, 1), dtype=np.uint32)
        given = None
        if part_of is not None:
            given = np.ascontiguousarray(part_of, dtype=np.uint32)
        h = C.c_void_p()
        check(self.lib.alz_plan_create_multi(arr, len(self.ctxs), _ref(lz), self.n, streams, _vp(given), C.byref(h), _vp(part)))
        self.h, self.part_of = h, part[:self.n]

    def execute(self, d_srcs, d_dsts):
        k = len(self.ctxs)
        a = (C.c_void_p * k)(*[p.value if hasattr(p, "value") else p for p in d_srcs])
        b = (C.c_void_p * k)(*[p.value if hasattr(p, "value") else p for p in d_dsts])
        check(self.lib.alz_plan_execute_multi(self.h, a, b))

    def results(self):
        res = (A.Result * self.n)()
        check(self.lib.alz_plan_results_multi(self.h, res))
        return res

    def close(self):
        if self.h:
            self.lib.alz_plan_destroy_multi(self.h)
            self.h = None


def layout_from_results(streams, results, align=16):
    """The second step of a two-pass decode: fills dst_off / dst_cap of `streams` from measured lengths (exclusive prefix sum, every stream's
    start rounded up to `align`) and returns the bytes the destination needs."""
    off = 0
    for s, r in zip(streams, results):
        off = (off + align - 1) // align * align
        s.dst_off, s.dst_cap = off, r.dst_len
        off += r.dst_len
    return off


def partition_batch(streams, n_parts):
    """alz_partition_batch: greedy LPT partition of a batch (host code, no GPU).  Returns (part_of np.uint32[n], cost np.uint64[n_parts])."""
    lib = load()
    n = len(streams)
    part = np.zeros(max(n, 1), dtype=np.uint32)
    cost = np.zeros(n_parts, dtype=np.uint64)
    check(lib.alz_partition_batch(n, streams, n_parts, _vp(part), _vp(cost)))
    return part[:n], cost


def decode_batch_multi(ctxs, streams, src, dst_bytes, lz=None):
    """alz_decode_batch_multi: ONE batch over several contexts (one per GPU; host threads inside the library)."""
    lib = load()
    n = len(streams)
    src = np.ascontiguousarray(src, dtype=np.uint8)
    dst = np.zeros(max(dst_bytes, 1), dtype=np.uint8)
    res = (A.Result * n)()
    part = np.zeros(max(n, 1), dtype=np.uint32)
    hs = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    check(lib.alz_decode_batch_multi(hs, len(ctxs), _ref(lz), n, _vp(src), src.nbytes, streams, _vp(dst), dst_bytes, res, _vp(part)))
    return dst, res, part[:n]


def encode_batch_multi(ctxs, streams, src, dst_bytes, quality=8, lz=None, strategy=0, min_distance=0, max_window_bits=0):
    """alz_encode_batch_multi: ONE batch of raw buffers over several contexts (one per GPU; host threads inside the library)."""
    lib = load()
    n = len(streams)
    src = np.ascontiguousarray(src, dtype=np.uint8)
    dst = np.zeros(max(dst_bytes, 1), dtype=np.uint8)
    res = (A.Result * n)()
    aux = _encode_aux(streams)
    part = np.zeros(max(n, 1), dtype=np.uint32)
    st = _settings(quality, strategy, min_distance, max_window_bits)
    hs = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
    check(lib.alz_encode_batch_multi(hs, len(ctxs), _ref(lz), st, n, _vp(src), src.nbytes, streams, _vp(dst), dst_bytes, res, aux, _vp(part)))
    return dst, res, aux, part[:n]
