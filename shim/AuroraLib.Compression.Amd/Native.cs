// Native.cs -- P/Invoke surface of libauroralz.so (include/auroralz.h, ALZ_ABI_VERSION 2).
// Every struct below mirrors a C struct field for field; tests/test_shim_binding.py parses this file and checks each
// [DllImport] (name, parameter count) and each struct (byte size) against the header, because no .NET SDK exists in the
// build image to compile it.  netstandard2.0-safe: UIntPtr instead of nuint, no Stream.ReadExactly, no function pointers.
using System;
using System.Runtime.InteropServices;

namespace AuroraLib.Compression.Amd
{
    /// <summary>alz_lz_properties (16 bytes) -- AuroraLib.Compression.LzProperties (LzProperties.cs:9-97) of the LZSS body.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct AlzLzProperties
    {
        public byte WindowBits;
        public byte LengthBits;
        public byte MinLength;
        public byte Reserved0;
        public uint WindowsStart;
        public uint MaxDistance;
        public uint Reserved1;
    }

    /// <summary>alz_stream (40 bytes): one stream of a batch; offsets are relative to the src / dst base of the call.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct AlzStream
    {
        public ulong SrcOff;
        public ulong DstOff;
        public uint SrcLen;
        public uint DstCap;
        public uint DecomLen;
        public uint Aux0;
        public uint Aux1;
        public uint Format;
    }

    /// <summary>alz_result (16 bytes).</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct AlzResult
    {
        public uint DstLen;
        public uint SrcUsed;
        public int Status;
        public uint Reserved;
    }

    /// <summary>alz_settings (16 bytes) -- CompressionSettings (CompressionSettings.cs:11-84).</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct AlzSettings
    {
        public int Quality;
        public int MaxWindowBits;
        public int Strategy;
        public int MinDistance;
    }

    /// <summary>alz_encode_aux (8 bytes): Yay0 / MIO0 section offsets of an encoded stream.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct AlzEncodeAux
    {
        public uint Aux0;
        public uint Aux1;
    }

    /// <summary>alz_file_result (16 bytes): what the single-file call returns for one file of an alz_zfile_* or alz_framed_* batch.</summary>
    [StructLayout(LayoutKind.Sequential, Size = 16)]
    public struct AlzFileResult
    {
        public int Rc;
        public int Status;
        public uint DstLen;
        public uint SrcUsed;
    }

    /// <summary>alz_format: the headerless bodies (values are ABI constants).</summary>
    public enum AlzFormat : uint
    {
        LZSS = 0, LZ10 = 1, LZ11 = 2, Yaz0 = 3, Yay0 = 4, MIO0 = 5, PrsBE = 6, PrsLE = 7, LZ4Block = 8, LZO = 9, SnappyRaw = 10,
        LZ40 = 11, LZHudson = 12, SMSR00 = 13, FastLZ = 14, CNX2 = 15, BLZ = 16, CLZ0 = 17, CNS = 18, LZ02 = 19, RefPack = 20,
        WFLZ = 21, WFLZ_BE = 22, LZShrek = 23, HIG = 24
    }

    /// <summary>alz_status: the reference's exception classes as per-stream codes (INTEGRATION.md section 3).</summary>
    public enum AlzStatus : int { Ok = 0, InputTruncated = 1, OutputSizeMismatch = 2, OutputCapacity = 3, BadToken = 4 }

    /// <summary>alz_container values used by the framed formats of this assembly.</summary>
    public enum AlzContainer : uint { Snappy = 9, LZ4Frame = 22 }

    internal static unsafe class Native
    {
        private const string Lib = "auroralz";   // libauroralz.so / auroralz.dll on the loader path

        [DllImport(Lib)] internal static extern int alz_abi_version();
        [DllImport(Lib)] internal static extern int alz_device_count();
        [DllImport(Lib)] internal static extern int alz_create(int device, out IntPtr ctx);
        [DllImport(Lib)] internal static extern void alz_destroy(IntPtr ctx);
        [DllImport(Lib)] internal static extern IntPtr alz_last_error();
        [DllImport(Lib)] internal static extern int alz_ctx_set_exact_kernels(IntPtr ctx, int on);
        [DllImport(Lib)] internal static extern int alz_ctx_release_scratch(IntPtr ctx);
        [DllImport(Lib)] internal static extern int alz_ctx_big_stream(IntPtr ctx, uint minBytes, ulong* launchesOut);

        // one stream: backs Decompress(Stream, Stream) of one format class
        [DllImport(Lib)] internal static extern int alz_decode(IntPtr ctx, uint format, AlzLzProperties* props,
            byte* src, uint srcLen, uint decomLen, uint aux0, uint aux1, byte* dst, uint dstCap, AlzResult* result);

        // many streams: the batched form of BruteForceCommand's RawDecoder delegate (CLI/Commands/BruteForceCommand.cs:88-133)
        [DllImport(Lib)] internal static extern int alz_decode_batch(IntPtr ctx, AlzLzProperties* props, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);

        // decoded sizes without decoding: results[i] is what alz_decode_batch would return for streams[i]; dst_off is ignored, dst_cap bounds the count
        [DllImport(Lib)] internal static extern int alz_measure_batch(IntPtr ctx, AlzLzProperties* props, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);

        // ... on a source that is already in HBM (dSrcBase is a device pointer)
        [DllImport(Lib)] internal static extern int alz_measure_batch_device(IntPtr ctx, AlzLzProperties* props, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);

        // RLE30 / HUF20, the non-LZ bodies of the GBA / DS family: AlzStream.format holds an alz_rlh_format (0 RLE30, 1 HUF20 4-bit, 2 HUF20 8-bit);
        // aux0 of a 4-bit stream is the nibble order (1 = Endian.Big, Level5).  HUF20 has no encoder (ALZ_E_UNSUPPORTED).
        [DllImport(Lib)] internal static extern int alz_rlh_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_rlh_decode_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_rlh_encode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_rlh_encode_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);

        // aPLib (Formats/Common/aPLib.cs), decode only: headerless bodies in batches (format, decomLen, aux0, aux1 of a stream are ignored; the body
        // ends at its end marker), their sizes without decoding, and the aPLib class on an "AP32" file or a headerless body in host memory
        [DllImport(Lib)] internal static extern int alz_aplib_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_aplib_decode_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_aplib_measure_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_aplib_measure_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_aplib_is_match(byte* src, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_aplib_decompressed_size(byte* src, UIntPtr srcLen, uint* sizeOut);
        [DllImport(Lib)] internal static extern int alz_aplib_decompress(IntPtr ctx, byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap,
            UIntPtr* dstLen, UIntPtr* srcUsed, int* status);

        // CRILAYLA (CRI/CRILAYLA.cs) and ALLZ (Specialized/ALLZ.cs), decode only: headerless bodies in batches (AlzStream.format is an alz_bitlz_kind:
        // 0 CRILAYLA -- written from dstOff + dstCap down --, 1 ALLZ -- decomLen and aux0 = copy | dist << 8 | len << 16 start bits), and the two
        // classes on a whole file in host memory
        [DllImport(Lib)] internal static extern int alz_bitlz_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_bitlz_decode_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_crilayla_is_match(byte* src, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_crilayla_decompressed_size(byte* src, UIntPtr srcLen, uint* sizeOut);
        [DllImport(Lib)] internal static extern int alz_crilayla_decompress(IntPtr ctx, byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap,
            UIntPtr* dstLen, UIntPtr* srcUsed, int* status);
        [DllImport(Lib)] internal static extern int alz_allz_is_match(byte* src, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_allz_decompressed_size(byte* src, UIntPtr srcLen, uint* sizeOut);
        [DllImport(Lib)] internal static extern int alz_allz_decompress(IntPtr ctx, byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap,
            UIntPtr* dstLen, UIntPtr* srcUsed, int* status);

        // CRILAYLA and ALLZ written on the GPU (CompressHeaderless of the two classes, the managed bytes for the same settings): raw buffers in
        // batches (AlzStream.format is an alz_bitlz_kind, an ALLZ stream's aux0 its three start bits; the body occupies [dstOff, dstOff + dstLen)),
        // and the two classes' files, one or a batch.  ALLZ at quality 1 is refused (ALZ_E_UNSUPPORTED); CRILAYLA.Compress / ALLZ.Compress stay managed
        [DllImport(Lib)] internal static extern UIntPtr alz_bitenc_bound(uint kind, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_bitenc_encode_batch(IntPtr ctx, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_bitenc_encode_batch_device(IntPtr ctx, AlzSettings* settings, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern UIntPtr alz_bitenc_file_bound(uint kind, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_bitenc_file_compress(IntPtr ctx, uint kind, AlzSettings* settings, uint aux0,
            byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap, UIntPtr* dstLen);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_bitenc_file_compress_batch(IntPtr ctx, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);

        // aPLib written on the GPU (aPLib.CompressHeaderless, the managed bytes for the same settings): raw buffers in batches (format, decomLen, aux0,
        // aux1 of a stream are ignored; the body occupies [dstOff, dstOff + dstLen)) and "AP32" files, one or a batch.  An empty source is
        // ALZ_E_INVALID; at qualities 1..7 a source longer than the managed chain table is ALZ_E_UNSUPPORTED; aPLib.Compress stays managed
        [DllImport(Lib)] internal static extern UIntPtr alz_apenc_bound(UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_apenc_encode_batch(IntPtr ctx, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_apenc_encode_batch_device(IntPtr ctx, AlzSettings* settings, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern UIntPtr alz_apenc_file_bound(UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_apenc_file_compress(IntPtr ctx, AlzSettings* settings,
            byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap, UIntPtr* dstLen);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_apenc_file_compress_batch(IntPtr ctx, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);

        // DEFLATE as zlib's inflate reads it (the body of ZLib / GZip, which the managed classes hand to the BCL), decode only: raw streams in
        // batches (format, decomLen, aux0, aux1 of a stream are ignored), their sizes without decoding, and the two classes on a whole file in
        // host memory (checksums verified on the host; *_measure takes them as correct)
        [DllImport(Lib)] internal static extern int alz_inflate_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_inflate_decode_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_inflate_measure_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_inflate_measure_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_zlib_is_match(byte* src, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_gzip_is_match(byte* src, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_zlib_decompress(IntPtr ctx, byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap,
            UIntPtr* dstLen, UIntPtr* srcUsed, int* status);
        [DllImport(Lib)] internal static extern int alz_gzip_decompress(IntPtr ctx, byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap,
            UIntPtr* dstLen, UIntPtr* srcUsed, int* status);
        [DllImport(Lib)] internal static extern int alz_zlib_measure(IntPtr ctx, byte* src, UIntPtr srcLen, UIntPtr sizeLimit,
            UIntPtr* sizeOut, UIntPtr* srcUsed, int* status);
        [DllImport(Lib)] internal static extern int alz_gzip_measure(IntPtr ctx, byte* src, UIntPtr srcLen, UIntPtr sizeLimit,
            UIntPtr* sizeOut, UIntPtr* srcUsed, int* status);

        // Adler-32 (kind 0) and CRC-32 (kind 1) of byte ranges on the GPU (a range is SrcOff / SrcLen of its AlzStream) ...
        [DllImport(Lib)] internal static extern int alz_checksum_batch(IntPtr ctx, uint kind, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* ranges, uint* checksums);
        [DllImport(Lib)] internal static extern int alz_checksum_batch_device(IntPtr ctx, uint kind, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* ranges, uint* checksums);
        // ... the checksum of A || B from those of A and B (host arithmetic), and ZLib (format 0) / GZip (format 1) files in batches: per
        // file what alz_zlib_decompress / alz_gzip_decompress return for it alone
        [DllImport(Lib, ExactSpelling = true)] internal static extern uint alz_checksum_combine(uint kind, uint a, uint b, ulong lenB);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_zfile_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_zfile_measure_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, AlzFileResult* results);

        // XXH32 (the checksum of the LZ4 frame format) of byte ranges on the GPU: the argument rules of alz_checksum_batch, a seed in place of the kind ...
        [DllImport(Lib)] internal static extern int alz_xxh32_batch(IntPtr ctx, uint seed, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* ranges, uint* hashes);
        [DllImport(Lib)] internal static extern int alz_xxh32_batch_device(IntPtr ctx, uint seed, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* ranges, uint* hashes);
        // ... and LZ4 (frame 22, legacy 7) / framed Snappy (9) files in batches: AlzStream.Format is the alz_container value; per file what
        // alz_container_decompress / alz_container_measure return for it alone
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_framed_decode_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_framed_measure_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, AlzFileResult* results);

        // CRC-32C (Castagnoli; a framed Snappy chunk's checksum before its mask) of byte ranges on the GPU: the argument rules of
        // alz_checksum_batch without a kind, and the join of two neighbouring pieces on the host
        [DllImport(Lib)] internal static extern int alz_crc32c_batch(IntPtr ctx, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* ranges, uint* sums);
        [DllImport(Lib)] internal static extern int alz_crc32c_batch_device(IntPtr ctx, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* ranges, uint* sums);
        [DllImport(Lib, ExactSpelling = true)] internal static extern uint alz_crc32c_combine(uint a, uint b, ulong lenB);
        // LZ4 (frame 22, legacy 7) / framed Snappy (9) files WRITTEN in batches: the multi-block containers BatchEncoder.CompressMany cannot
        // serve body by body.  AlzStream.Format is the alz_container value, Aux0 an LZ4 frame's block size; per file what
        // alz_container_compress writes and returns for it alone
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_framing_compress_batch(IntPtr ctx, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);

        // DEFLATE WRITTEN on the GPU: raw streams (level 0..9 with zlib's meaning, flags bit 0 = fixed Huffman codes only) and ZLib (kind 0) /
        // GZip (kind 1) files, one or a batch (AlzStream.Format is the kind).  The library's own encoder: valid streams, not the bytes a BCL
        // would write, so ZLib.Compress / GZip.Compress stay managed
        [DllImport(Lib)] internal static extern UIntPtr alz_deflate_bound(UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_deflate_block_bytes();
        [DllImport(Lib)] internal static extern int alz_deflate_encode_batch(IntPtr ctx, int level, uint flags, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern int alz_deflate_encode_batch_device(IntPtr ctx, int level, uint flags, uint n,
            byte* dSrcBase, UIntPtr srcBytes, AlzStream* streams, byte* dDstBase, UIntPtr dstBytes, AlzResult* results);
        [DllImport(Lib)] internal static extern UIntPtr alz_deflate_file_bound(uint kind, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_deflate_file_compress(IntPtr ctx, uint kind, int level, uint flags,
            byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap, UIntPtr* dstLen);
        [DllImport(Lib, ExactSpelling = true)] internal static extern int alz_deflate_file_compress_batch(IntPtr ctx, int level, uint flags, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* files, byte* dstBase, UIntPtr dstBytes, AlzFileResult* results);

        // decompressed size of a file of a container without a size field (PRS, LZO, FastLZ, LZ4 frame / legacy, framed Snappy), measured on the GPU
        [DllImport(Lib)] internal static extern int alz_container_measure(IntPtr ctx, uint container, void* opt,
            byte* src, UIntPtr srcLen, UIntPtr sizeLimit, UIntPtr* sizeOut, UIntPtr* srcUsed, int* status);

        // the same batch over several contexts (one per GPU), partitioned by the library
        [DllImport(Lib)] internal static extern int alz_decode_batch_multi(IntPtr* ctxs, uint nCtx, AlzLzProperties* props, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results, uint* partOfOut);

        [DllImport(Lib)] internal static extern int alz_partition_batch(uint n, AlzStream* streams, uint nParts, uint* partOf, ulong* partCost);

        // CompressHeaderless of every format class + LzChainMatchFinder (bit-identical to the managed encoder at every quality)
        [DllImport(Lib)] internal static extern int alz_encode_batch(IntPtr ctx, AlzLzProperties* props, AlzSettings* settings, uint n,
            byte* srcBase, UIntPtr srcBytes, AlzStream* streams, byte* dstBase, UIntPtr dstBytes, AlzResult* results, AlzEncodeAux* aux);

        // whole-file helpers of the framed formats (LZ4 frame: descriptor, xxHash32 checksums, linked blocks; Snappy framing: CRC-32C)
        [DllImport(Lib)] internal static extern int alz_container_decompress(IntPtr ctx, uint container, void* opt, byte* src, UIntPtr srcLen,
            byte* dst, UIntPtr dstCap, UIntPtr* dstLen, UIntPtr* srcUsed, int* status);
        [DllImport(Lib)] internal static extern int alz_container_compress(IntPtr ctx, uint container, void* opt, AlzSettings* settings,
            byte* src, UIntPtr srcLen, byte* dst, UIntPtr dstCap, UIntPtr* dstLen);
        [DllImport(Lib)] internal static extern UIntPtr alz_container_compress_bound(uint container, UIntPtr srcLen);
        [DllImport(Lib)] internal static extern int alz_container_decompressed_size(uint container, void* opt, byte* src, UIntPtr srcLen, uint* sizeOut);
    }
}
