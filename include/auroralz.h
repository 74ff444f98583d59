/*
 * auroralz.h -- C ABI of the MI355X-native batched LZ codec ("auroralz").
 *
 * This is the drop-in boundary for the LZ match-copy hot path of
 * Venomalia/AuroraLib.Compression.  The reference is pure managed C# and has
 * no FFI of its own; every entry point below replaces one managed interface
 * of the reference (cited as file:line under /root/reference) and is what a
 * C# `[DllImport("auroralz")]` shim binds.
 *
 * Rules of the ABI: extern "C", plain pointers and sizes, POD structs with
 * fixed-width fields, no ownership crosses the boundary (the caller owns all
 * src/dst buffers; the library owns its device scratch inside alz_ctx /
 * alz_plan).  Functions return 0 on success or a negative ALZ_E_* code for API
 * level failures (bad argument, HIP failure, no device).  Per-stream decode
 * outcomes are reported in alz_result.status (ALZ_ST_*), mirroring the
 * reference's exceptions.
 *
 * There is NO CPU fallback behind this ABI: every decode/encode runs on the
 * GPU through the hand-written gfx950 kernels.  Without a device alz_create()
 * fails with ALZ_E_NO_DEVICE.
 */
#ifndef AURORALZ_H
#define AURORALZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALZ_ABI_VERSION 2

/* ---- formats: the headerless bodies on the hot path ---- */
typedef enum alz_format {
    ALZ_FMT_LZSS       = 0,  /* LZSS.DecompressHeaderless    src/AuroraLib.Compression/Formats/Common/LZSS.cs:91-130   */
    ALZ_FMT_LZ10       = 1,  /* LZ10.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/LZ10.cs:82-111 */
    ALZ_FMT_LZ11       = 2,  /* LZ11.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/LZ11.cs:83-133 */
    ALZ_FMT_YAZ0       = 3,  /* Yaz0.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/Yaz0.cs:91-92 (Yay0 body, one cursor) */
    ALZ_FMT_YAY0       = 4,  /* Yay0.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/Yay0.cs:99-144 (three cursors) */
    ALZ_FMT_MIO0       = 5,  /* MIO0.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/MIO0.cs:105-149 */
    ALZ_FMT_PRS_BE     = 6,  /* PRS.DecompressHeaderless(.., Endian.Big)    src/AuroraLib.Compression.Sega/Sega/PRS.cs:59-102 */
    ALZ_FMT_PRS_LE     = 7,  /* PRS.DecompressHeaderless(.., Endian.Little) same body, LSB-first flags + LE u16 */
    ALZ_FMT_LZ4_BLOCK  = 8,  /* LZ4.DecompressBlockHeaderless src/AuroraLib.Compression/Formats/Common/LZ4.cs:176-200 */
    ALZ_FMT_LZO        = 9,  /* LZO.DecompressHeaderless     src/AuroraLib.Compression/Formats/Common/LZO.cs:49-139 */
    ALZ_FMT_SNAPPY_RAW = 10, /* Snappy.DecompressHeaderless  src/AuroraLib.Compression/Formats/Common/Snappy.cs:205-250 */
    ALZ_FMT_LZ40       = 11, /* LZ40.DecompressHeaderless    src/AuroraLib.Compression.Nintendo/Nintendo/LZ40.cs:80-132 (also the body of LZ60) */
    ALZ_FMT_LZHUDSON   = 12, /* LZHudson.DecompressHeaderless: the Yay0 grammar on ONE stream with 32-bit big-endian flag words
                                src/AuroraLib.Compression.Nintendo/HudsonSoft/LZHudson.cs:53 */
    ALZ_FMT_SMSR00     = 13, /* SMSR00.DecompressHeaderless: u16 BE codes (16-bit masks + MIO0 tokens) | literals; aux0 = length of the
                                code section   src/AuroraLib.Compression.Nintendo/Nintendo/SMSR00.cs:70-131 */
    ALZ_FMT_FASTLZ     = 14, /* FastLZ.DecompressHeaderless (levels 1 and 2; the level is the top 3 bits of the first byte)
                                src/AuroraLib.Compression/Formats/Common/FastLZ.cs:54-160.  SURVEY.md 8f rank 4. */
    ALZ_FMT_CNX2       = 15, /* CNX2.DecompressHeaderless: 2-bit codes (skip / literal / match / literal run), 2 KiB window
                                src/AuroraLib.Compression.Sega/Sega/CNX2.cs:83-139.  SURVEY.md 8f rank 4. */
    ALZ_FMT_BLZ        = 16, /* BLZ.DecompressHeaderless in stream order: the managed code walks both spans from their ends
                                (src/AuroraLib.Compression.Nintendo/Nintendo/BLZ.cs:97-135), so `src` is the code section REVERSED and
                                `dst` receives the output REVERSED (alz_container_* does both reversals); decom_len = the length of
                                the destination span.  SURVEY.md 8f rank 4. */
    ALZ_FMT_CLZ0       = 17, /* CLZ0.DecompressHeaderless: LZSS family, flags LSB first with 1 = match, distance = 0x1000 - delta
                                src/AuroraLib.Compression-Extended/Marvelous/CLZ0.cs:64-97.  SURVEY.md 8f rank 4. */
    ALZ_FMT_CNS        = 18, /* CNS.DecompressHeaderless: control byte < 0x80 = that many literals, else a match of (c & 0x7F) + 3 bytes
                                at distance next byte + 1; 256-byte window
                                src/AuroraLib.Compression-Extended/Specialized/CNS.cs:77-108.  SURVEY.md 8f rank 4. */
    ALZ_FMT_LZ02       = 19, /* LZ02.DecompressHeaderless: flags MSB first, 1 = match (DDDDLLLL DDDDDDDD [+ length byte]), ends at the
                                terminator token, not at the declared size
                                src/AuroraLib.Compression-Extended/Camelot/LZ02.cs:77-115.  SURVEY.md 8f rank 4. */
    ALZ_FMT_REFPACK    = 20, /* RefPack.DecompressHeaderless: prefix byte + 1-3 data bytes = 0-3 literals + a match (three forms), 0xE0-0xFB =
                                4-112 literals, 0xFC-0xFF = 0-3 literals and the end; 128 KiB window; the declared size is only
                                compared at the end   src/AuroraLib.Compression-Extended/EA/RefPack.cs:177-245.  SURVEY.md 8f rank 4. */
    ALZ_FMT_WFLZ       = 21, /* WFLZ.DecompressHeaderless(.., Endian.Little): 4-byte blocks (u16 distance, length - 4, literal count) each
                                followed by its literals; block 0/0/0 ends the stream
                                src/AuroraLib.Compression-Extended/WayForward/WFLZ.cs:130-159.  SURVEY.md 8f rank 4. */
    ALZ_FMT_WFLZ_BE    = 22, /* WFLZ.DecompressHeaderless(.., Endian.Big): the same body with big-endian distance words */
    ALZ_FMT_LZSHREK    = 23, /* LZShrek.DecompressHeaderless: groups of (flag: literal count | match count - 1) + literals + 1..8 matches with
                                variable-length length / distance fields; ends at a zero length byte; 4 KiB window (a distance beyond it --
                                encodable, but the managed decoder wraps it around its ring -- is BAD_TOKEN)
                                src/AuroraLib.Compression-Extended/Activision/LZShrek.cs:73-119.  SURVEY.md 8f rank 4. */
    ALZ_FMT_HIG        = 24, /* HIG.DecompressHeaderless: an initial literal block, then matches (three forms, lengths to 65 535, 32 KiB
                                window) each followed by 0 / 1 / 2 / counted literals
                                src/AuroraLib.Compression-Extended/Specialized/HIG.cs:126-212.  SURVEY.md 8f rank 4. */
    ALZ_FMT_COUNT      = 25
} alz_format;

/* ---- per-stream status: the reference's exception types ---- */
typedef enum alz_status {
    ALZ_ST_OK                   = 0,
    ALZ_ST_INPUT_TRUNCATED      = 1, /* EndOfStreamException / IndexOutOfRangeException */
    ALZ_ST_OUTPUT_SIZE_MISMATCH = 2, /* DecompressedSizeException (LZ10.cs:107-110 '>', LZSS.cs:126-129 '!=') */
    ALZ_ST_OUTPUT_CAPACITY      = 3, /* NotSupportedException of a fixed-size destination */
    ALZ_ST_BAD_TOKEN            = 4  /* reference-undefined input the library refuses: see E3 below */
} alz_status;

/*
 * E3 -- a match distance beyond the window W of its format (encodable by Snappy's 4-byte-offset copy against its 64 KiB
 * LzWindows, Snappy.cs:244-247 / :213, and by LZShrek's distances up to 65 822 against its 4 KiB one) -- is REFUSED with
 * ALZ_ST_BAD_TOKEN; every other body cannot encode one.  A decision against SURVEY.md 8a-1, which froze E3 as "d mod W in
 * Release": reading LzWindows.BackCopy (IO/LzWindows.cs:72-100) and InternWrite (:192-227) shows that the masked source
 * position (`srcPos = (_Position - distance) & mask`) is what "d mod W" describes only while the masked distance is at least the
 * chunk of the pass (`chunk = min(length, distance, W - srcPos)`: for distance > W nothing keeps it below the masked distance).
 * Otherwise BackCopy hands Unsafe.CopyBlockUnaligned (cpblk) a source span that OVERLAPS its destination inside the ring -- a
 * case ECMA-335 leaves unspecified (forward copy on one runtime, memmove on another): the managed Release output for such a token
 * is not a function of the stream, so there is nothing to be bit-exact with.  Debug builds assert (:75).  The oracle and both kernel
 * families agree on the refusal (tests/cases.py, tests/golden/kat_*.json); valid streams never contain such a token.
 * E1 (distance 0 = W), E2 (sources before the stream start read 0x00), E4 / E5 (overshoot of the declared size / of dst_cap) are
 * as SURVEY.md 8a-1 froze them.
 */

/* ---- API-level error codes ---- */
#define ALZ_OK            0
#define ALZ_E_INVALID    -1  /* bad argument */
#define ALZ_E_NO_DEVICE  -2  /* no HIP device / runtime */
#define ALZ_E_HIP        -3  /* a HIP call failed; see alz_last_error() */
#define ALZ_E_NOMEM      -4
#define ALZ_E_UNSUPPORTED -5
#define ALZ_E_FORMAT     -6  /* container header invalid (InvalidIdentifierException) */
#define ALZ_E_STREAM     -7  /* single-stream helper: per-stream status != OK (status is returned separately) */
#define ALZ_E_CHECKSUM   -8  /* LZ4 frame block / content checksum mismatch (InvalidDataException, LZ4.Frame.cs:22-28) */

/*
 * LzProperties of the generic LZSS body (src/AuroraLib.Compression/LzProperties.cs:9-97).
 * Only consulted for ALZ_FMT_LZSS streams; all other formats have fixed geometry.
 * Defaults (all zero) mean LZSS.DefaultProperties = LzProperties((byte)12, 4, 2)
 * (LZSS.cs:33): window_bits 12, length_bits 4, min_length 3, windows_start 0xFEE.
 */
typedef struct alz_lz_properties {
    uint8_t  window_bits;    /* LzProperties.WindowsBits  (7..16 supported on the GPU path) */
    uint8_t  length_bits;    /* LzProperties.LengthBits   */
    uint8_t  min_length;     /* LzProperties.MinLength    */
    uint8_t  reserved0;
    uint32_t windows_start;  /* LzProperties.WindowsStart */
    uint32_t max_distance;   /* LzProperties.MaxDistance  (== 1 << window_bits for the bit-based ctor) */
    uint32_t reserved1;
} alz_lz_properties;

/*
 * One stream of a batch.  Offsets are relative to the src_base / dst_base
 * passed to the batch call, so one descriptor table serves host and device
 * resident buffers alike.
 *
 * decom_len : the `decomLength` argument of the reference's DecompressHeaderless
 *             (LZSS/LZ10/LZ11/LZ40/YAZ0/YAY0/MIO0/LZHUDSON/SMSR00).  Ignored by PRS/LZ4/LZO (no size
 *             field, terminated by token / end of input) and by SNAPPY_RAW
 *             (varint inside the body).
 * aux0/aux1 : YAY0/MIO0: compressedDataPointer / uncompressedDataPointer
 *             relative to the first flag byte (Yay0.cs:60, MIO0.cs:61).
 *             SMSR00: aux0 = bytes of the code section (the literal section follows it).
 *             LZ4_BLOCK: aux0 = history, the number of bytes in front of dst_off
 *             (<= dst_off) that are earlier output of the same LZ4 frame and may
 *             be referenced by matches -- one LzWindows serves all blocks of a
 *             frame (LZ4.Frame.cs:120).  0 = a fresh window (LZ4.cs:164).
 * dst_cap   : bytes the library may write at dst_off.  Never exceeded.
 */
typedef struct alz_stream {
    uint64_t src_off;
    uint64_t dst_off;
    uint32_t src_len;
    uint32_t dst_cap;
    uint32_t decom_len;
    uint32_t aux0;
    uint32_t aux1;
    uint32_t format;     /* alz_format */
} alz_stream;

typedef struct alz_result {
    uint32_t dst_len;    /* bytes written at dst_off (<= dst_cap) */
    uint32_t src_used;   /* source bytes consumed; the reference leaves source.Position there
                            (Yay0.cs:89-90, MIO0.cs:92-93, LZSS.cs:68).  OK / OUTPUT_SIZE_MISMATCH / BAD_TOKEN: just behind the
                            last token read.  INPUT_TRUNCATED: src_len (the reader ran into the end of the input).
                            OUTPUT_CAPACITY: unspecified (the managed code throws from inside LzWindows' write to the
                            caller's fixed-size stream; nothing reads Position after that). */
    int32_t  status;     /* alz_status */
    uint32_t reserved;
} alz_result;

/* CompressionSettings (src/AuroraLib.Compression/CompressionSettings.cs:11-84) */
typedef struct alz_settings {
    int32_t quality;          /* 0..15; presets Fastest 0, Fast 4, Balanced 8 (default), High 12, Maximum 15 */
    int32_t max_window_bits;  /* 0 = auto.  The managed finder only ever WIDENS its window with it (windowsBits = max(format,
                               * MaxWindowBits), maxDistance = max(format, 1 << MaxWindowBits); MatchFinder/LzChainMatchFinder.cs:
                               * 69-73), so a value within the format's own window is accepted and changes nothing.  A larger one
                               * is taken for FastLZ (> 13 selects level 2 for sources >= 64 KiB at quality > 4, Formats/Common/
                               * FastLZ.cs:169-175) up to 20 -- the finder on the device keeps a distance in 21 bits -- and refused
                               * (ALZ_E_UNSUPPORTED) otherwise: the managed finder would return distances the format cannot store */
    int32_t strategy;         /* 0 Default, 1 CompatibilityMode (no self-overlapping matches) */
    int32_t min_distance;     /* 0 = format default; 2 = LZ10/LZ11 GbaVramCompatibilityMode (LZ10.cs:25-33) */
} alz_settings;

typedef struct alz_ctx  alz_ctx;   /* one HIP device + one HIP stream; single-threaded */
typedef struct alz_plan alz_plan;  /* a prepared batch: descriptors resident in HBM, grouped per format */

/* ---------------------------------------------------------------- context */
int         alz_abi_version(void);
int         alz_device_count(void);
int         alz_create(int device, alz_ctx** out);
void        alz_destroy(alz_ctx* ctx);
const char* alz_last_error(void);          /* thread-local text of the last failure */
int         alz_device_info(alz_ctx* ctx, char* name, size_t name_cap, int* cu_count, uint64_t* hbm_bytes);
/* Kernel family of a context.  0 (default): the lane-parallel production kernels.  1: the exact kernels -- one token at a
 * time, the statement-for-statement GPU restatement of the managed bodies; every lane-parallel kernel hands its stream
 * tails and error paths to them.  A verification mode (the parity tests run every case through both families). */
int         alz_ctx_set_exact_kernels(alz_ctx* ctx, int on);
/* Several production kernels exist in two shapes: one wavefront per stream (a full GPU: most streams resident) and two --
 * one parses, one copies -- for launches that cannot fill the GPU anyway (a lone stream, a small batch).  0 (default): the
 * library chooses by the size of the batch; 1 / 2: always the one- / two-wavefront shape where both exist.  Results are
 * identical; a tuning and verification hook (the library reads no environment variable for kernel selection).
 * A third shape exists for the flag-byte family (LZSS with windows up to 4 KiB, LZ10, LZ11, LZ40, CLZ0, Yaz0, Yay0, MIO0) and PRS on device-resident
 * plans: the batch as a WORK QUEUE of (stream, chunk) items -- 40 KiB of output per chunk, PRS 80 KiB --, ONE workgroup per item, each drawing its item as a ticket from the queue head
 * when it starts -- taken by itself (variant 0) when a plan has more streams of such a format than 0.4 of what the GPU holds of that format's wavefronts (and more than fit the two-wavefront
 * shape: half the GPU's places; PRS: more than the GPU holds), so that the launch does not end in a partly filled round; 3: plans created in this
 * mode use it whatever their size (the parity tests).  Same results: a chunk ends between two iterations of the lane-parallel loop and hands
 * the LDS window and the cursors on.  An item waits for the chunk before its own; tickets are drawn in start order, so that chunk is always in the hands of a workgroup that is
 * already running (progress does not depend on the order in which the hardware dispatches workgroups).  The wait is still a BOUNDED spin; if one ever ran out (a fault: never
 * seen) a sticky word of the plan is set, and the gated launch that alz_plan_execute enqueues behind every queue launch decodes that format's streams again with one wavefront
 * per stream -- on the same stream, in order: work the caller chained behind the execute sees whole output either way.  alz_plan_results then moves the plan off the queue. */
int         alz_ctx_set_kernel_variant(alz_ctx* ctx, int variant);
/* ONE big stream: a batch of one -- or of a few, as long as one after the other on the whole GPU beats side by side on wavefronts of their
 * own -- LZSS / LZ10 / LZ11 / Yaz0 / Yay0 / MIO0 / PRS / LZO / LZ4-block / raw-Snappy streams (all eleven
 * north-star bodies) of at least `min_bytes` of output each (default 24 KiB -- where the two cross: ONE stream of 32 KiB takes 0.18 ms here and 0.30 on its wavefront, of 256 KiB 0.20 and 1.3; PRS / LZO / LZ4 / Snappy, which carry no size in the
 * descriptor: of dst_cap, with at least 8 KiB of input) is decoded
 * stream by stream by the whole GPU instead of by one or two wavefronts per stream (csrc/alz_big.hip).  Yay0 / MIO0 keep flags, match tokens
 * and literals in three sections (Yay0.cs:99-108, MIO0.cs:105-116): every token's cursors are prefix sums.  The other four interleave them
 * in one byte stream, but what a group of eight tokens (LZ4: a sequence, Snappy: an element, PRS: the tokens behind one flag byte, per
 * entry state of its control-bit automaton; LZO: an instruction, per class of the literal count before it) that started at byte p WOULD occupy is a function of the bytes behind p alone, so the real starts are found by list ranking over the input bytes.  Either way the copies are resolved by pointer jumping over the
 * output bytes.  So the single-stream call a format class's Decompress(Stream, Stream) makes (Interfaces/ICompressionDecoder.cs:24; the
 * reference's own benchmark is ONE 1 000 KiB stream, Benchmarks/Benchmarks/TestAllAlgorithms.cs:41-42) does not fall behind the managed
 * decoder.  Results are identical: a stream that path cannot finish -- any malformed one -- is decoded by the exact kernel behind it.
 * The ENCODER has the same switch (csrc/alz_encode_big.h): an alz_encode_batch / _device call of at most 32 buffers, each of at least
 * 8 KiB (or `min_bytes`, if that is less: the batch pipeline gives a buffer one workgroup and one wavefront, and loses from 8 KiB on) of one of these formats (and LZ40 / CLZ0 / BLZ / LZHudson; distances within 16 bits), is compressed buffer by buffer on the whole
 * GPU -- prev() on overlapping segments, the greedy / lazy parse (FindNextBestMatch, MatchFinder/LzChainMatchFinder.cs:157-212) as list ranking
 * over "where would a cursor at p go", the emission by prefix sums -- instead of by one workgroup and one wavefront per buffer: what
 * a format class's Compress(ReadOnlySpan<byte>, Stream) makes of ONE buffer (Interfaces/ICompressionEncoder.cs; the reference's benchmark
 * compresses ONE 1 000 KiB buffer, TestAllAlgorithms.cs:44-69).  The bytes are the same either way.
 * Between the two -- more buffers than that, fewer than fill the GPU with a wavefront each (1 280 / 1 536 / 512 of a format per call at quality 0 / 1-10 / 11-15), the longest
 * of at least 8 KiB: the chunks of one archive, a directory of files -- the flag-bit formats with a bounded match length (LZSS, LZ10, Yaz0, Yay0, MIO0, CLZ0, BLZ, LZHudson),
 * raw Snappy and PRS parse from one synchronisation point of the walk to the next (a position no jump crosses) with a wavefront each and emit per segment
 * (csrc/alz_encode_seg.h).  No switch: the bytes are the same, and a context in exact or forced-variant mode never goes that way.
 * min_bytes: 0 keeps the current threshold, 0xFFFFFFFF switches both paths off; launches_out (may be NULL) receives how many streams the two paths have TAKEN on this
 * context: the decode side counts on the device, where the path decides -- a stream it declines (any malformed one) is decoded by the kernel behind the gate and NOT counted --,
 * and asking waits for everything enqueued on the device so far.  Contexts in exact or forced-variant mode (alz_ctx_set_exact_kernels / alz_ctx_set_kernel_variant) never take them. */
int         alz_ctx_big_stream(alz_ctx* ctx, uint32_t min_bytes, uint64_t* launches_out);
/* The host-buffer entry points keep their device staging buffers and the encoder's scratch (per input byte: a 16- or 32-bit link
 * in a 32-bit slot -- above quality 0 a second one, the links of the finder's wider hash narrowed from 15-bit ones --, a 32-bit
 * match entry -- not at quality 0 for the formats whose search runs inside their emit kernel --, two bytes of section buffers for
 * Yay0 / MIO0 / SMSR00, one bit of start mask for the formats without a parallel emitter; the finder's head tables live in LDS) in
 * the context and only ever grow them, so that a caller
 * working through batch after batch does not pay a device allocation per call.  This returns all of it to the device (the
 * managed side has no counterpart: ArrayPool<int>.Shared keeps LzChainMatchFinder's tables the same way,
 * MatchFinder/LzChainMatchFinder.cs:85-104, :323-334). */
int         alz_ctx_release_scratch(alz_ctx* ctx);

/* ----------------------------------------------- decode: host buffers in/out
 * Replaces the loop a managed caller writes around the static
 * `DecompressHeaderless(Stream source, Stream destination, uint decomLength)`
 * bodies -- the uniform raw-decoder delegate of
 * src/AuroraLib.Compression.CLI/Commands/BruteForceCommand.cs:88-133.
 * src_base/dst_base are HOST pointers; the call uploads, decodes on the GPU,
 * downloads and returns.  `props` may be NULL (LZSS defaults). */
int alz_decode_batch(alz_ctx* ctx, const alz_lz_properties* props, uint32_t n,
                     const uint8_t* src_base, size_t src_bytes,
                     const alz_stream* streams,
                     uint8_t* dst_base, size_t dst_bytes,
                     alz_result* results);

/* The same call over several contexts = several GPUs of one node: the batch is partitioned by
 * alz_partition_batch, each share is packed, uploaded, decoded and downloaded by its own host thread on its own context
 * (one context per device; ctxs[] must not repeat a context), no collective -- streams are independent (a fresh LzWindows
 * per Decompress call, src/AuroraLib.Compression.Nintendo/Nintendo/LZ10.cs:86).  part_of_out (may be NULL) receives the
 * index into ctxs[] that decoded stream i.  Results are identical to alz_decode_batch on any one of the contexts. */
int alz_decode_batch_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, uint32_t n,
                           const uint8_t* src_base, size_t src_bytes,
                           const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes,
                           alz_result* results, uint32_t* part_of_out);
/* Greedy LPT partition of a batch over n_parts devices, balanced by decompressed bytes x a per-format cost (the host-side
 * partitioning of SURVEY.md 8e).  part_of[i] = part of stream i; part_cost[n_parts] (may be NULL) = the load of each part.
 * Pure host code: one process per GPU (bench.py --scaling strong) uses it to pick its share of ONE batch. */
int alz_partition_batch(uint32_t n, const alz_stream* streams, uint32_t n_parts, uint32_t* part_of, uint64_t* part_cost);

/* Single stream: backs ICompressionDecoder.Decompress(Stream, Stream) of one format class
 * (src/AuroraLib.Compression/Interfaces/ICompressionDecoder.cs:24) after the managed shim parsed the header. */
int alz_decode(alz_ctx* ctx, uint32_t format, const alz_lz_properties* props,
               const uint8_t* src, uint32_t src_len, uint32_t decom_len, uint32_t aux0, uint32_t aux1,
               uint8_t* dst, uint32_t dst_cap, alz_result* result);

/* ---------------------------------------- measure: decoded sizes without decoding
 * PRS, LZ4 blocks, LZO, FastLZ, WFLZ and raw Snappy carry no size a caller could read before the call, and every batch entry
 * point wants dst_off / dst_cap for every stream first.  The measure kernels walk a stream's tokens as the decoder does and
 * count: results[i] is what alz_decode_batch would return for streams[i] -- status, dst_len, and src_used wherever it is
 * defined (every status but OUTPUT_CAPACITY) -- for all formats.  dst_off is ignored, no destination exists, nothing is written
 * on the device but the results.  dst_cap only bounds the count: pass 0xFFFFFF00 for "the size", or a limit of your own to have a
 * stream that decodes to more end in ALZ_ST_OUTPUT_CAPACITY (dst_len = that limit).  An LZ4 block with history (aux0) counts like one
 * without (E2: bytes in front of a stream are zeros at worst, never an error), so the blocks of a linked frame can be measured
 * as one batch.  Two passes then lay a batch out exactly: sizes, exclusive prefix sum, alz_plan_create + execute.
 * alz_ctx_set_exact_kernels selects the family (the counting sink under the exact parsers alone / lane-parallel parse rounds
 * for the bulk of the size-less bodies); alz_last_kernel_ms reports the device time of the call's launches. */
int alz_measure_batch(alz_ctx* ctx, const alz_lz_properties* props, uint32_t n,
                      const uint8_t* src_base, size_t src_bytes, const alz_stream* streams, alz_result* results);
/* the same on a source that is already in HBM: d_src_base is a DEVICE pointer (typed as the bytes the offsets count, like src_base
 * above; 64 readable bytes behind the last stream, as for the plans below); results come back to the host */
int alz_measure_batch_device(alz_ctx* ctx, const alz_lz_properties* props, uint32_t n,
                             const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams, alz_result* results);

/* ---------------------------------------- RLE30 / HUF20: the non-LZ bodies of the Nintendo GBA / DS family
 * The BIOS family that LZ10 / LZ11 belong to has two members without a window: run-length (type 0x30) and Huffman (types 0x24 /
 * 0x28).  They are no alz_format -- no match copy, no LzWindows, no body in the CPU oracle -- and have an entry-point family of
 * their own, as measure has.  alz_stream and alz_result are reused: `format` holds an alz_rlh_format; aux0 is, for
 * ALZ_RLH_HUF20_4, the nibble order (0 = Endian.Little: HUF20 and LZ77; 1 = Endian.Big: Level5) and otherwise ignored, aux1 is
 * ignored.  The slack rules are those of the plans: 64 readable bytes behind the last stream of both device buffers, never a
 * write outside [dst_off, dst_off + dst_cap).  alz_ctx_set_exact_kernels selects the kernel family (one token / one bit at a
 * time against the lane-parallel kernels); alz_last_kernel_ms reports the device time of the call's launches.
 *
 * RLE30.DecompressHeaderless (Nintendo/RLE30.cs:76-105): control byte c, n = (c & 0x7F) + 1; c >= 0x80: the next byte n + 2
 *   times (3..130), else n literals (1..128).  Input that ends at a control byte, at a run byte or inside a literal run:
 *   INPUT_TRUNCATED, src_used = src_len, dst_len = the whole tokens before it (the managed code reads a literal run into a
 *   temporary and throws before it writes).  The last token may overshoot decom_len: written, OUTPUT_SIZE_MISMATCH (E4, the '>'
 *   rule of :101).  A token that would exceed dst_cap is clipped and ends decoding (E5, as LZ10).  decom_len 0: OK, nothing read.
 *   (These are also the rules of RLHudson, alz_rlhudson_* below: the same kernels over another grammar.)
 * RLE30.CompressHeaderless (:110-129 over MatchFinder/RleMatchFinder.cs:29-64, minMatch 3, maxMatch 127): bit-identical to the managed
 *   bytes INCLUDING ITS DEFECT (E7): 127 literals followed by fewer than 3 bytes become ONE literal run of up to 129 bytes
 *   (`duration = source.Length - offset`, RleMatchFinder.cs:43), whose control byte wraps to 0x80 -- such a stream does not decode
 *   back (129 or 256 non-repeating bytes; 128 and 130 round-trip).  Over dst_cap: OUTPUT_CAPACITY, dst_len 0.
 * HUF20.DecompressHeaderless (Nintendo/HUF20.cs:94-152): byte 0 treeSize, byte 1 treeRoot, treeSize * 2 tree bytes (a short read
 *   leaves zeros and is no error), then little-endian 32-bit words consumed MSB first; decom_len * 8 / bitDepth symbols.  4-bit
 *   mode ORs the WHOLE tree byte, shifted by 4 or 0, into a cleared destination: a leaf value above 0xF pollutes or loses bits
 *   exactly as the managed code does.  A missing header byte or word: INPUT_TRUNCATED, src_used = src_len; an index beyond the
 *   tree (IndexOutOfRangeException): INPUT_TRUNCATED, src_used just behind the last word read; a stream that decodes into
 *   dst_cap < decom_len: OUTPUT_CAPACITY (a stream error wins over it).  The managed code hands its destination nothing unless
 *   the whole decode succeeded (:103-107): dst_len = 0 for EVERY non-OK status, the bytes inside [dst_off, dst_off +
 *   min(dst_cap, decom_len)) are then unspecified, and nothing outside is written.  decom_len 0 still reads the header and the
 *   tree.  decom_len >= 0x10000000 is refused with ALZ_E_UNSUPPORTED (the managed `int` symbol count overflows).
 * HUF20 HAS NO ENCODER: alz_rlh_encode_batch* with a HUF format, and alz_container_compress of every HUF type, answer
 *   ALZ_E_UNSUPPORTED.  The project's bar is bit-identity with the managed encoder, and the managed output is not a function of
 *   the input that can be restated: HuffmanTree.CreateTree (Huffman/HuffmanTree.cs:89-101) orders equal frequencies with the
 *   UNSTABLE List.Sort() over a comparer that looks at Frequency only (HuffmanNode.cs:66-67), and the 4-bit path indexes its
 *   16-entry table with un-shifted high nibbles (HUF20.cs:189-196). */
typedef enum alz_rlh_format { ALZ_RLH_RLE30 = 0, ALZ_RLH_HUF20_4 = 1, ALZ_RLH_HUF20_8 = 2, ALZ_RLH_COUNT = 3 } alz_rlh_format;
int alz_rlh_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                         uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_rlh_decode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
/* src_* describe the raw input, dst_* the compressed output capacity (2 * src_len always suffices); results[i].dst_len is the compressed size */
int alz_rlh_encode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                         uint8_t* dst_base, size_t dst_bytes, alz_result* results);
int alz_rlh_encode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);

/* ---------------------------------------- RLHudson: Hudson Soft's byte RLE, the sibling of RLE30
 * RLHudson (src/AuroraLib.Compression.Nintendo/HudsonSoft/RLHudson.cs) is RLE30 with the other polarity and no length bias.  It is
 * NOT a fourth alz_rlh_format (ALZ_RLH_COUNT stays 3 and alz_rlh_decode_batch refuses format 3): it is a family with one kind and
 * entry points of its own, as aPLib has.  alz_stream and alz_result are reused; `format`, aux0 and aux1 of a stream are IGNORED.
 * Parameter lists, slack rules, the context modes (alz_ctx_set_exact_kernels: one token per step against the lane-parallel rounds,
 * the same two kernels as RLE30 over another grammar) and alz_last_kernel_ms are those of alz_rlh_*.
 *
 * RLHudson.DecompressHeaderless (:54-81): control byte c, n = c & 0x7F; c < 0x80: the next byte n times, else n literals.  n MAY BE
 *   0: `00 xx` consumes two bytes and `80` one, and neither writes anything.  Everything else is RLE30's rule set above, and for the
 *   same reasons: input that ends at a control byte (ReadByte() = -1 reads as a run of 127 whose ReadUInt8 throws), at a run byte or
 *   inside a literal run (the short read throws before anything is written): INPUT_TRUNCATED, src_used = src_len, dst_len = the
 *   whole tokens before it.  The last token may overshoot decom_len: written, OUTPUT_SIZE_MISMATCH (the '>' rule of :77).  A token
 *   that would exceed dst_cap is clipped and ends decoding (E5, statuses as RLE30).  decom_len 0: OK, nothing read.
 * RLHudson.CompressHeaderless (:83-102 over RleMatchFinder(3, 0x7F)): bit-identical to the managed bytes INCLUDING ITS DEFECT, which
 *   is RLE30's E7: `duration = source.Length - offset` (RleMatchFinder.cs:43) yields literal runs of 128 or 129 bytes, whose control
 *   bytes (byte)(duration | 0x80) come out as 0x80 / 0x81 -- such a stream does not decode back (128, 129 or 255 non-repeating
 *   bytes; 127 and 130 round-trip).  Over dst_cap: OUTPUT_CAPACITY, dst_len 0.  alz_rlhudson_encode_bound(src_len) always suffices.
 * The RLHudson FILE (8-byte header: u32 BE size, u32 BE 5) is ALZ_WF_RLHUDSON of the alz_wfile_* family below. */
int alz_rlhudson_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                              uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_rlhudson_decode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                     uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
/* src_* describe the raw input, dst_* the compressed output capacity; results[i].dst_len is the compressed size */
int alz_rlhudson_encode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                              uint8_t* dst_base, size_t dst_bytes, alz_result* results);
int alz_rlhudson_encode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                     uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
size_t alz_rlhudson_encode_bound(size_t src_len);   /* 2 * src_len: no token has more bytes than twice what it covers */

/* ---------------------------------------- aPLib: the last LzWindows user of the reference (decode only)
 * aPLib (src/AuroraLib.Compression/Formats/Common/aPLib.cs) is no alz_format: its body carries no size, ends at an end marker and looks
 * back up to W = 0x200000 (2 MiB, WindowsBits 21); it has no body in the CPU oracle.  It has an entry-point family of its own, as measure
 * and rlh have.  alz_stream and alz_result are reused; decom_len, aux0, aux1 and format of a stream are IGNORED.  The slack rules are
 * those of alz_rlh_* and the plans (64 readable bytes behind the last stream of both device buffers, never a write outside
 * [dst_off, dst_off + dst_cap)).  Two kernel families with identical results: alz_ctx_set_exact_kernels(1) selects the exact one (one token
 * at a time), alz_ctx_set_kernel_variant(1) the token-queue kernel with the lane-parallel byte phase; a context in neither mode gets the one
 * that was measured faster (docs/EXPERIMENTS.md 13).  alz_last_kernel_ms reports the device time of the call's launch.
 *
 * aPLib.DecompressHeaderless (aPLib.cs:105-181): the first byte is a literal; then tokens, each introduced by up to three 1-bits from a
 * FlagReader(source, Endian.Big) -- 8-bit flag bytes, MSB first, fetched lazily at the current input position when a bit is needed and
 * none is left, so flag bytes and data bytes interleave: `0` literal byte; `10` gamma-coded match (or, right behind a literal / one-byte
 * token, gamma 2 = repeat the last distance); `110` byte b: distance b >> 1, length 2 + (b & 1), distance 0 = the END MARKER; `111` four
 * bits o: one byte from distance o, o == 0 writes 0x00.  The edge rules:
 *   32-bit arithmetic  ReadGamma and (offset << 8) | byte are C# ints in an unchecked context: computed in uint32_t, read as int32_t; the
 *                      repeat test `offset == 2` sees the wrapped value.
 *   distance           negative as int32_t or larger than W: ALZ_ST_BAD_TOKEN (E3).  The length gamma behind it is read first, as the managed
 *                      code does before BackCopy: src_used is just behind that gamma; input that ends inside it is INPUT_TRUNCATED.
 *   length             after LengthDelta, as int32_t: <= 0 copies nothing (LzWindows.cs:80; lastOffset and lwm are still updated), anything
 *                      positive is legal and clipped by dst_cap (E5).
 *   distance 0         (a repeat before any match; a match with high part 0 and low byte 0) copies from W back (E1); sources in front of
 *                      the stream start read 0x00 (E2).
 *   end of input       a missing flag or data byte: INPUT_TRUNCATED, dst_len = what was produced, src_used = src_len.  Empty input:
 *                      INPUT_TRUNCATED, dst_len 0.
 *   capacity           a literal or match that does not fit dst_cap is clipped: OUTPUT_CAPACITY, dst_len = dst_cap, src_used unspecified.
 *   success            OK means the end marker was read; src_used is just behind its byte.
 * alz_aplib_measure_batch*: results[i] is what alz_aplib_decode_batch would return for streams[i] -- status, dst_len, and src_used wherever
 *   it is defined (every status but OUTPUT_CAPACITY); dst_off is ignored, dst_cap only bounds the count (0xFFFFFF00 for "the size"),
 *   nothing is written on the device but the results.
 * THERE IS NO ENCODER in this family: the writer is alz_apenc_* below.  aPLib.CompressHeaderless runs the tiered LzChainMatchFinder over
 *   seven LzProperties with a 2 MiB window and unbounded lengths; the CPU oracle has no aPLib, so bit-identity with the managed bytes is held
 *   against a Python restatement.  alz_brute_force and alz_container_scan keep their 19 decoders / alz_container values and do not try aPLib
 *   (INTEGRATION.md). */
int alz_aplib_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_aplib_decode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                  uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
int alz_aplib_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                            alz_result* results);
int alz_aplib_measure_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                   alz_result* results);
/* The aPLib class (aPLib.cs:39-84) on a whole file in host memory.
 * alz_aplib_is_match: 1 when src_len > 0x10, the magic "AP32" and u32 LE at offset 4 == 24 (IsMatchStatic, :44), else 0.
 * alz_aplib_decompressed_size: u32 LE at offset 16; ALZ_E_FORMAT without the magic or with fewer than 20 bytes.
 * alz_aplib_decompress: without the magic at offset 0 (or with fewer than 4 bytes) the whole input is a headerless body (:59-64).
 *   With it, 24 header bytes are needed (else ALZ_E_FORMAT) and the body starts at 24 + ((headerSize - 24) mod 2^32), computed in 64
 *   bits as the managed `Position += uint` is: a header size below 24 lands beyond the end -- ALZ_E_STREAM / INPUT_TRUNCATED, *dst_len 0.
 *   The compressed-size field is only traced by the reference and ignored here.  A decoded size different from the header's:
 *   ALZ_E_STREAM / OUTPUT_SIZE_MISMATCH with *dst_len the actual size.  *src_used = body start + the body's src_used.  On
 *   ALZ_E_STREAM, *status holds the alz_status. */
int alz_aplib_is_match(const uint8_t* src, size_t src_len);
int alz_aplib_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out);
int alz_aplib_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                         size_t* dst_len, size_t* src_used, int32_t* status);

/* ---------------------------------------- CRILAYLA and ALLZ: the bit-stream LZ bodies of the .Extended assembly (decode only)
 * CRILAYLA (src/AuroraLib.Compression-Extended/CRI/CRILAYLA.cs, CRI Middleware's CPK compression) and ALLZ
 * (src/AuroraLib.Compression-Extended/Specialized/ALLZ.cs, Aqualead LZ) are no alz_format values: neither has a body in the CPU oracle.
 * They share an entry-point family of their own.  alz_stream and alz_result are reused; streams[i].format is an alz_bitlz_kind, any other
 * value makes the call return ALZ_E_INVALID; a batch may mix both kinds (one launch per kind present).  The slack rules are those of
 * alz_aplib_* (64 readable bytes behind the last stream of both device buffers).  Each kind has ONE kernel, the exact one, so
 * alz_ctx_set_exact_kernels, alz_ctx_set_kernel_variant and a context in neither mode give identical results by construction.
 * alz_last_kernel_ms reports the device time of the call's launches.  The kernels READ the input in aligned 8- and 16-byte granules: up to
 * 15 bytes below src_off inside its 16-byte granule (never across a page) and up to 64 bytes behind src_off + src_len; the only other
 * reads are of the stream's own output.
 *
 * CRILAYLA body (DecompressHeaderless, CRILAYLA.cs:123-188).  src_len = the compressed bytes, dst_cap = the length of the destination span
 * (the file layer passes size + 0x100); decom_len, aux0, aux1 are ignored.  The bit source starts at the LAST input byte and moves towards
 * the first; within a byte bits are taken MSB first, values are assembled MSB first across bytes.  OUTPUT BYTE q, counted from 0, GOES TO
 * dst_off + dst_cap - 1 - q.  Tokens, read while unread input bytes remain (bits left in the last loaded byte are padding of either value):
 * `0` + 8 bits: a literal; `1` + 13 bits + length code: a match of distance field + 3 (3..8194) and length 3 + the sum of fields of
 * 2, 3, 5, 8, 8, ... bits, where a field of all ones continues (3-5 | 6-12 | 13-43 | 44-298 | 299-553 | ...); out[q] = out[q - distance]
 * byte by byte, so overlap replicates.
 *   distance > bytes produced   ALZ_ST_BAD_TOKEN, nothing copied; the length code is read first; src_used = bytes loaded so far.
 *   does not fit dst_cap        a literal or match is clipped: OUTPUT_CAPACITY, dst_len = dst_cap, src_used unspecified (BAD_TOKEN is checked first).
 *   input ends inside a token   INPUT_TRUNCATED; the token produces nothing; dst_len = what earlier tokens produced; src_used = src_len.
 *   empty input                 OK, 0 bytes.
 *   success                     OK, src_used = src_len; the dst_len bytes occupy [dst_off + dst_cap - dst_len, dst_off + dst_cap) and nothing
 *                               below that is written (whatever the status); the match length is summed in 64 bits.
 * ALLZ body (DecompressHeaderless, ALLZ.cs:90-127).  decom_len = the destination span, dst_cap = what may be written,
 * aux0 = ALZ_ALLZ_AUX0(flags[1], flags[2], flags[3]): the start bits of match length / distance / run length (class defaults 0 / 10 / 1).
 * FlagReader(source, Endian.Little): 8-bit flag bytes, LSB first, fetched at the CURRENT input position when a bit is needed and none is
 * left, so flag bytes and raw run bytes interleave and bits left in a flag byte stay valid across a run.  ReadALFlag(s): bits = s, plus one
 * per 1-bit up to the first 0-bit; then `bits` bits, least significant first; then + ((1 << (bits - s)) - 1) << s -- all in C# int
 * arithmetic (32-bit wrap, shift counts mod 32, `1 << i` in ReadInt too), read as int32_t.  While produced < decom_len: one bit, `0`: a run of
 * ReadALFlag(len) + 1 raw bytes from the input, `1`: no run; then, if still produced < decom_len, distance = ReadALFlag(dist) + 1,
 * length = ReadALFlag(copy) + 3 and a byte-wise copy from produced - distance (the window is the whole output so far).
 *   run < 0                     BAD_TOKEN.  run == 0 copies nothing.
 *   match length <= 0           copies nothing and is no error, whatever the distance.
 *   length > 0 and distance <= 0 or > produced    BAD_TOKEN, src_used just behind the length field (a match as the first token too).
 *   passes min(decom_len, dst_cap)   a run or match is clipped there: OUTPUT_CAPACITY when dst_cap < decom_len, else OUTPUT_SIZE_MISMATCH;
 *                               src_used unspecified for both.
 *   a needed flag byte is missing, or the input holds fewer bytes than a run (after clipping) needs: INPUT_TRUNCATED, src_used = src_len;
 *                               the run bytes that exist are copied.
 *   decom_len 0                 OK, nothing read.       success: OK, dst_len == decom_len, src_used = the input position.
 * THE ENCODER is alz_bitenc_* below.  The CPU oracle has neither body, so its bit-identity with the managed bytes is held against a Python
 *   restatement of LzChainMatchFinder and of the two CompressHeaderless bodies, and that restatement is pinned to the oracle through the formats
 *   the oracle does have.  alz_brute_force and alz_container_scan do not try the two formats. */
typedef enum alz_bitlz_kind { ALZ_BITLZ_CRILAYLA = 0, ALZ_BITLZ_ALLZ = 1, ALZ_BITLZ_COUNT = 2 } alz_bitlz_kind;
#define ALZ_ALLZ_AUX0(copy_bits, dist_bits, len_bits)  ((copy_bits) | (dist_bits) << 8 | (len_bits) << 16)   /* flags[1], flags[2], flags[3] */
int alz_bitlz_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_bitlz_decode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                  uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
/* The CRILAYLA class (CRILAYLA.cs:34-99) on a whole file in host memory: "CRILAYLA", u32 LE size at 8, u32 LE csize at 12, the body of csize
 * bytes at 16, then 0x100 plain header bytes.
 * alz_crilayla_is_match: 1 when src_len > 0x10 and the magic, else 0.
 * alz_crilayla_decompressed_size: size + 0x100 computed in uint32_t; ALZ_E_FORMAT without the magic or with fewer than 12 bytes.
 * alz_crilayla_decompress: fewer than 16 bytes or no magic: ALZ_E_FORMAT.  size + 0x100 >= 2^31: ALZ_E_UNSUPPORTED (the managed (int) cast).
 *   csize reaches beyond the input: ALZ_E_STREAM / INPUT_TRUNCATED, *dst_len 0.  dst_cap < size + 0x100: ALZ_E_STREAM / OUTPUT_CAPACITY,
 *   *dst_len 0, nothing decoded.  Otherwise the output is size + 0x100 bytes: [0, 0x100) are the plain header bytes behind the body (missing
 *   ones 0x00), the body is decoded over the top of the span and wins where it reaches into the header region (:81), bytes that neither
 *   wrote are 0x00.  A body that produced fewer than `size` bytes: ALZ_E_STREAM / OUTPUT_SIZE_MISMATCH with *dst_len = size + 0x100 and the
 *   bytes delivered (the managed code writes before it throws, :86-92).  Body errors pass through as ALZ_E_STREAM with their status.
 *   *src_used = 16 + csize + min(0x100, what is left). */
int alz_crilayla_is_match(const uint8_t* src, size_t src_len);
int alz_crilayla_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out);
int alz_crilayla_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                            size_t* dst_len, size_t* src_used, int32_t* status);
/* The ALLZ class (ALLZ.cs:39-75): "ALLZ", 4 flag bytes (byte 0 unused), u32 LE size at 8, the body at 12.
 * alz_allz_is_match: 1 when src_len > 0x10 and the magic.  alz_allz_decompressed_size: the u32 at 8; ALZ_E_FORMAT without the magic or with
 * fewer than 12 bytes.  alz_allz_decompress: the body with decom_len = size (fewer than 12 bytes or no magic: ALZ_E_FORMAT; a size the
 * managed (int) cast makes negative: ALZ_E_UNSUPPORTED); *src_used = 12 + the body's; on ALZ_E_STREAM, *status holds the alz_status. */
int alz_allz_is_match(const uint8_t* src, size_t src_len);
int alz_allz_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out);
int alz_allz_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status);

/* ---------------------------------------- CRILAYLA and ALLZ written: CompressHeaderless of the two classes (CRILAYLA.cs:190-258, ALLZ.cs:129-174)
 * Both bodies run LzChainMatchFinder, so the encoder's finder kernels serve them: the bytes are those of the managed code for the same
 * CompressionSettings.  streams[i].format is an alz_bitlz_kind (anything else: ALZ_E_INVALID); a batch may mix both kinds.  src_* is the raw
 * input, dst_* where the body goes: it occupies [dst_off, dst_off + dst_len) -- CRILAYLA's too, which the managed code writes from the end of
 * its array downwards: the bytes are the same.  alz_result is { OK, dst_len, src_used = src_len }; a body that does not fit dst_cap is
 * ALZ_ST_OUTPUT_CAPACITY with dst_len 0, and nothing outside [dst_off, dst_off + dst_cap) is ever written.  alz_bitenc_bound(kind, n) is the
 * worst case of the body and always suffices: 9 n / 8 for CRILAYLA, which is tight.  For ALLZ it is LOOSE, about 5.9 n: it knows neither
 * aux0 nor the data and charges every three source bytes a unit of maximal fields (a bound from aux0 and the 2^19 distance limit would be
 * several times tighter: not built).  A caller short of memory may give a smaller dst_cap and handle ALZ_ST_OUTPUT_CAPACITY.  The file layer
 * sizes its slots by the bound.
 * settings: NULL = quality 8.  quality outside 0..15: ALZ_E_INVALID.  max_window_bits other than 0, and min_distance other than 0:
 *   ALZ_E_UNSUPPORTED (the managed finder would return what neither format stores).  ALLZ AT QUALITY 1 IS ALZ_E_UNSUPPORTED: maxChain is 2
 *   and the managed chain table has 2^18 slots for a 2^19 window, so its links are not what the kernels compute (LzChainMatchFinder.cs:94-96);
 *   every other quality 0..15 is supported for both kinds.
 * CRILAYLA: LzProperties(0x2000, 65535, 3, 0, 3); the finder runs over the REVERSED source (:204-206), reversed on the device.  aux0 ignored.
 * ALLZ: five tiered LzProperties, a 512 KiB window, lengths to 0x40000.  aux0 = ALZ_ALLZ_AUX0(copy, dist, len), each 0..24, else
 *   ALZ_E_INVALID.  src_len above 0x40000000: ALZ_E_UNSUPPORTED (within it WriteALFlag's int sums do not wrap).  Empty input: the byte 01.
 * One wavefront writes one stream's bits, placed by prefix sums; alz_ctx_set_exact_kernels selects the form in which one lane writes them token
 *   by token: the same bytes.  A lone large buffer goes through the same batch pipeline as many small ones: neither format has a whole-GPU
 *   path or a segmented walk.  The device form needs no slack behind its source (streams at the buffer's end are
 *   copied to scratch, as alz_encode_batch_device does).  alz_last_kernel_ms reports the device time of the call's launches.
 * The file layer, host memory.  kind is an alz_bitlz_kind.
 *   CRILAYLA (Compress, :102-121): a source under 0x100 bytes is ALZ_E_INVALID.  "CRILAYLA", u32 LE src_len - 0x100, u32 LE csize, the body of
 *     source[0x100:], then source[:0x100].  The managed class rents src_len + 10 % for the body and fails where nine bits per literal (12.5 %)
 *     run out of it; the library writes the file a large enough array would have given.  aux0 ignored.
 *   ALLZ (Compress, :78-88): "ALLZ", { 0, copy, dist, len } from aux0, u32 LE src_len, the body.
 *   alz_bitenc_file_compress: a dst_cap that is too small is ALZ_E_NOMEM (*dst_len 0); alz_bitenc_file_bound(kind, n) suffices.
 *   alz_bitenc_file_compress_batch: files[i].format the kind, files[i].aux0 ALLZ's start bits; all bodies of the call are ONE
 *     alz_bitenc_encode_batch.  results[i] is { ALZ_OK, ALZ_ST_OK, dst_len, src_len } and the bytes of the single-file call on file i alone,
 *     or { that call's code, ALZ_ST_OK, 0, 0 }: one file's failure is that file's rc, nothing outside a file's slot is written.
 * NOT BUILT: device-resident file forms, shim classes.  (aPLib, the third bit-stream body, is written by alz_apenc_* below.) */
size_t alz_bitenc_bound(uint32_t kind, size_t src_len);
int alz_bitenc_encode_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                            const alz_stream* streams, uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_bitenc_encode_batch_device(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                                   const alz_stream* streams, uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
struct alz_file_result;                            /* (defined with alz_zfile_* below) */
size_t alz_bitenc_file_bound(uint32_t kind, size_t src_len);
int alz_bitenc_file_compress(alz_ctx* ctx, uint32_t kind, const alz_settings* settings, uint32_t aux0, const uint8_t* src, size_t src_len,
                             uint8_t* dst, size_t dst_cap, size_t* dst_len);
int alz_bitenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                   const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, struct alz_file_result* results);

/* ---------------------------------------- aPLib written: aPLib.CompressHeaderless and Compress (Formats/Common/aPLib.cs:183-286, :87-103)
 * The body alz_aplib_* reads, written with the managed code's bytes for the same CompressionSettings.  Every stream of a call is one body:
 * format, aux0, aux1 and decom_len of a stream are IGNORED.  src_* is the raw input, dst_* where the body goes; alz_result is
 * { OK, dst_len, src_used = src_len }; a body that does not fit dst_cap is ALZ_ST_OUTPUT_CAPACITY with dst_len 0 -- the body is sized before
 * it is written -- and nothing outside [dst_off, dst_off + dst_cap) is ever written.  alz_apenc_bound(n) = n + 1 + ceil((n + 2) / 8) for
 * n >= 1 (0 for 0) is the worst case, literals only, and is tight: no other token costs more than nine bits per byte it covers.
 * The finder: seven LzProperties in the class's order -- (0x1000, max, 3), (0x80, 3, 2), (0x4000, max, 4), (0x10000, max, 5), (0x40000, max, 6),
 *   (0x100000, max, 7), (0x200000, max, 8): ScoreMatch takes the first that admits a candidate --, minimum length 2, a 2 MiB window; a match at
 *   distance exactly 0x200000 is found and written.
 * The body: source[0] raw, then FlagWriter(Endian.Big) -- 8-bit flag bytes, most significant bit first, payload bytes behind the flag byte
 *   that was open when they were handed over.  A byte outside a match is `111` + 4 bits (the byte is 0: offset 0; it equals one of the
 *   min(16, position + 1) - 1 bytes in front of it: the nearest such offset 1..15) or `0` + the byte.  A match is a repeat (`10`, gamma 2,
 *   gamma L: no match ended right here and the distance is the last one), a short block (`11` + byte D << 1 | L - 2: L <= 3, D <= 127) or a
 *   normal block (`10`, gamma (D >> 8) + 2, + 1 unless a match ended right here, byte D & 0xFF, gamma L - LengthDelta(D)).  The end: `11`, byte 0, `0`.
 * settings: NULL = quality 8.  quality outside 0..15: ALZ_E_INVALID.  max_window_bits other than 0, and min_distance other than 0:
 *   ALZ_E_UNSUPPORTED.  strategy 0 and 1 (noSelfOverlap) are both supported.  QUALITIES 1..7 NEED SHORT STREAMS: the managed chain table has
 *   1 << min(17 + floor(sqrt(2 q)), 21) slots -- 2^18 at quality 1, 2^19 at 2..4, 2^20 at 5..7 -- for a 2^21 window, and once a slot is reused its
 *   links are not what the kernels compute (LzChainMatchFinder.cs:94-96).  A call at one of these qualities in which any stream is longer than
 *   that many bytes is ALZ_E_UNSUPPORTED, decided before anything is uploaded (alz_last_error says which stream); qualities 0 and 8..15 have
 *   no such condition.
 * A stream with src_len 0 makes the call ALZ_E_INVALID, before anything is uploaded: the managed code throws on source[0].  src_len above
 *   0x40000000: ALZ_E_UNSUPPORTED.  n == 0: ALZ_OK.
 * One wavefront writes one stream's bits, a lane per position, placed by prefix sums; alz_ctx_set_exact_kernels selects the form in which one
 *   lane writes them token by token: the same bytes.  A lone large buffer goes through the same batch pipeline as many small ones (no
 *   whole-GPU path, no segmented walk).  The device form needs no slack behind its source.  alz_last_kernel_ms reports the device time of the
 *   call's launches.
 * The file layer, host memory (Compress, :87-103): "AP32", then u32 LE 24, the body's size, 0, src_len, 0 (both CRC fields are written as 0),
 *   then the body.  alz_apenc_file_bound(n) = 24 + alz_apenc_bound(n) suffices.
 *   alz_apenc_file_compress: a dst_cap that is too small is ALZ_E_NOMEM (*dst_len 0); an empty source is ALZ_E_INVALID.
 *   alz_apenc_file_compress_batch: all bodies of the call are ONE alz_apenc_encode_batch.  results[i] is { ALZ_OK, ALZ_ST_OK, dst_len, src_len }
 *     and the bytes of the single-file call on file i alone, or { that call's code, ALZ_ST_OK, 0, 0 }: one file's failure (an empty file, a
 *     slot too small) is that file's rc, nothing outside a file's slot is written.  A condition on the whole call (the quality, the chain
 *     table's size at qualities 1..7) is the call's return value.
 * NOT BUILT: a whole-GPU or segmented path for one large buffer, device-resident file forms, a shim class, rows in alz_brute_force /
 *   alz_container_scan. */
size_t alz_apenc_bound(size_t src_len);
int alz_apenc_encode_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                           const alz_stream* streams, uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_apenc_encode_batch_device(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                                  const alz_stream* streams, uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
size_t alz_apenc_file_bound(size_t src_len);
int alz_apenc_file_compress(alz_ctx* ctx, const alz_settings* settings, const uint8_t* src, size_t src_len,
                            uint8_t* dst, size_t dst_cap, size_t* dst_len);
int alz_apenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                  const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, struct alz_file_result* results);

/* ---------------------------------------- DEFLATE: raw streams, their sizes, ZLib and GZip files (decode only)
 * The reference hands the bodies of its ZLib and GZip classes (src/AuroraLib.Compression/Formats/Common/ZLib.cs:30-34, GZip.cs:29-34) and
 * of the zlib wrappers of its .Extended assembly to the BCL, so there is no managed loop to restate: the contract is RFC 1950 / 1951 /
 * 1952 as zlib implements them.  DEFLATE is no alz_format and no alz_container: it has an entry-point family of its own, as aPLib has.
 * alz_stream and alz_result are reused; decom_len, aux0, aux1 and format of a stream are IGNORED.  The slack rules are those of
 * alz_aplib_* (64 readable bytes behind the last stream of both device buffers, never a write outside [dst_off, dst_off + dst_cap)).
 * One wavefront decodes one stream.  There is ONE decode kernel and ONE measure kernel, so alz_ctx_set_exact_kernels,
 * alz_ctx_set_kernel_variant and a context in neither mode give identical results by construction.  alz_last_kernel_ms reports the
 * device time of the call's launch.
 *
 * The raw body: zlib's `inflate` with window bits -15 and no dictionary.  Bits are packed LSB first; blocks are read until the one
 * with BFINAL ends.
 *   block type 3       ALZ_ST_BAD_TOKEN.
 *   stored block       the bits up to the byte boundary are dropped, LEN and NLEN are read; NLEN != ~LEN is BAD_TOKEN; LEN bytes are
 *                      copied (LEN 0 is legal).
 *   fixed block        literal/length symbols 286 and 287 and distance symbols 30 and 31 decode but are BAD_TOKEN when met.
 *   dynamic block      each of these is BAD_TOKEN, detected when the block header is parsed, even if the block holds no symbol:
 *                      HLIT + 257 > 286 or HDIST + 1 > 30; a code-length code that is over-subscribed or incomplete (one with no code at
 *                      all included); repeat code 16 with no previous length; a repeat that runs past HLIT + HDIST + 258 lengths; length
 *                      0 for symbol 256; a literal/length set or a distance set that is over-subscribed, or incomplete unless its longest
 *                      code is 1 bit (a single code).  A distance set with no code at all is legal; a code that a set does not have
 *                      (the unused code of a single-code set, any distance code of an empty set) is BAD_TOKEN when a stream uses it.  A
 *                      repeat may run from the literal/length lengths into the distance lengths.
 *   distance           larger than the bytes produced so far: BAD_TOKEN (nothing lies in front of a stream; the window is 32 KiB, the
 *                      largest distance a symbol can name).  It is tested before capacity.
 *   BAD_TOKEN          dst_len = what the symbols before the bad one produced; src_used unspecified.  The bits of a field are needed
 *                      before the field is judged: a malformed field that the input cuts short is INPUT_TRUNCATED.
 *   INPUT_TRUNCATED    the input ends before the final end-of-block.  dst_len = what the symbols whose bits are ALL present produced -- a
 *                      length code, its extra bits, the distance code and its extra bits count as one symbol; of a stored block the
 *                      bytes that exist are copied.  src_used = src_len.  Empty input: INPUT_TRUNCATED, dst_len 0.
 *   OUTPUT_CAPACITY    a literal, match or stored run that does not fit dst_cap is clipped: dst_len = dst_cap, src_used unspecified.  It
 *                      is raised only when a byte that does not fit is to be written (an end-of-block at dst_len == dst_cap is fine).
 *   OK                 the final end-of-block was read; src_used is just behind the byte that holds its last bit (the rest of that byte
 *                      is padding of either value).
 * alz_inflate_measure_batch*: results[i] is what alz_inflate_decode_batch would return for streams[i] -- status, dst_len, and src_used
 *   wherever it is defined; dst_off is ignored, dst_cap only bounds the count (0xFFFFFF00 for "the size"), nothing is written on the
 *   device but the results.
 * THE ENCODER is alz_deflate_* below (behind alz_zfile_*): the BCL's output depends on the zlib build behind it, so there are no managed
 *   bytes to be identical with, and its contract is the one above read backwards.  Preset
 *   dictionaries are not supported.  alz_brute_force and alz_container_scan do not try DEFLATE. */
int alz_inflate_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                             uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_inflate_decode_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                    uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
int alz_inflate_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                              alz_result* results);
int alz_inflate_measure_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                     alz_result* results);
/* The ZLib and GZip classes on a whole file in host memory.  Checksums are computed on the host over the downloaded output.  The header
 * walks need no context (a NULL ctx is ALZ_E_INVALID only once a body has to be decoded).
 * alz_zlib_is_match: ZLib.IsMatchStatic (ZLib.cs:26-27, :52-76) statement for statement: src_len > 4, CM == 8, CINFO <= 7,
 *   (CMF * 256 + FLG) % 31 == 0, the first block's type is not 3, and for type 0 the test as written -- LEN is read from the first two
 *   data bytes, is compared with its own complement and must not be 0.
 * alz_gzip_is_match: src_len > 8 and the bytes 1F 8B 08 (GZip.cs:25-26).
 * alz_zlib_decompress (RFC 1950): fewer than 2 bytes, CM != 8, CINFO > 7 or (CMF * 256 + FLG) % 31 != 0: ALZ_E_FORMAT; FDICT set:
 *   ALZ_E_UNSUPPORTED.  CINFO does not limit distances (zlib opened with 15 window bits behaves this way).  The body decodes as one
 *   stream; its errors pass through as ALZ_E_STREAM with their status and *src_used = 2 + the body's.  Fewer than 4 trailer bytes:
 *   ALZ_E_STREAM / INPUT_TRUNCATED with the output delivered, *src_used = src_len.  The trailer is the big-endian Adler-32 of the
 *   output: a mismatch is ALZ_E_CHECKSUM (the output is delivered).  *src_used = 2 + body + 4; bytes behind the trailer are not looked at.
 * alz_gzip_decompress (RFC 1952): magic or CM wrong, or a reserved FLG bit set: ALZ_E_FORMAT; a header that runs past the input:
 *   ALZ_E_STREAM / INPUT_TRUNCATED; FEXTRA, FNAME, FCOMMENT and FHCRC are skipped with bounds checks, FHCRC is verified against the low
 *   16 bits of the CRC-32 of the header (ALZ_E_CHECKSUM).  The trailer is the CRC-32 of the member's output and ISIZE, its length mod
 *   2^32: fewer than 8 bytes are ALZ_E_STREAM / INPUT_TRUNCATED with the output delivered, a mismatch of either is ALZ_E_CHECKSUM.
 *   Members follow one another while the next two bytes are 1F 8B: each is decoded by a call of its own and the outputs are
 *   concatenated (*dst_len counts all of them, also when a later member fails); any other trailing bytes end decoding without error.
 *   On success *src_used = src_len (the reference sets source.Position = source.Length, GZip.cs:33).
 * alz_zlib_measure / alz_gzip_measure: the alz_container_measure contract for these two classes -- rc, *status, *size_out (what
 *   *dst_len would be) and *src_used of reading the file into size_limit bytes, the bodies measured on the GPU, with the Adler-32 /
 *   CRC-32 taken as correct (they need the bytes; FHCRC and ISIZE are verified).  A size_limit below the true size gives
 *   ALZ_E_STREAM / ALZ_ST_OUTPUT_CAPACITY.
 * On ALZ_E_STREAM, *status holds the alz_status. */
int alz_zlib_is_match(const uint8_t* src, size_t src_len);
int alz_gzip_is_match(const uint8_t* src, size_t src_len);
int alz_zlib_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status);
int alz_gzip_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status);
int alz_zlib_measure(alz_ctx* ctx, const uint8_t* src, size_t src_len, size_t size_limit,
                     size_t* size_out, size_t* src_used, int32_t* status);
int alz_gzip_measure(alz_ctx* ctx, const uint8_t* src, size_t src_len, size_t size_limit,
                     size_t* size_out, size_t* src_used, int32_t* status);

/* ---------------------------------------- checksums of byte ranges: Adler-32 and CRC-32 on the GPU
 * out[i] is the checksum of the n ranges[i]: ALZ_CK_ADLER32 is RFC 1950's (zlib.adler32), ALZ_CK_CRC32 the CRC-32 with polynomial
 * 0xEDB88320, start value and final inversion 0xFFFFFFFF (zlib.crc32).  A range is src_off / src_len of its alz_stream; EVERY OTHER
 * FIELD IS IGNORED.  Ranges may overlap, be empty (Adler-32 1, CRC-32 0) and start at any byte.  The device writes nothing but the n
 * results (and the library's own scratch).  The kernels READ a range in aligned 16-byte granules -- never a granule that holds no byte
 * of a range -- so the slack rule of alz_aplib_* (64 readable bytes behind the buffer) covers them.
 * Every range is cut into chunks of 32 KiB; one wavefront sums one chunk, the grid runs over all chunks of all ranges, and a second,
 * small launch joins each range's chunk sums: many small ranges and one huge range fill the GPU alike.  alz_last_kernel_ms reports the
 * device time of the two launches.  n == 0 is ALZ_OK; a NULL ctx, an unknown kind, a range outside src_bytes, or NULL ranges / out with
 * n > 0 are ALZ_E_INVALID (checked before anything is uploaded); more than 2^31 chunks in one call are ALZ_E_UNSUPPORTED.
 * alz_checksum_combine: the checksum of A || B from the checksum `a` of A, the checksum `b` of B and the length of B (zlib's
 *   adler32_combine / crc32_combine): pure host code, no context, the very arithmetic the second launch runs.  len_b == 0 returns a.
 *   An unknown kind returns 0.
 * NOT BUILT: a checksum fused into a decode kernel's write-back.  CRC-32C, the checksum of the Snappy container, and XXH32, the checksum
 *   of the LZ4 frame format, have entry points of their own below (alz_crc32c_batch*, alz_xxh32_batch*). */
typedef enum alz_checksum_kind { ALZ_CK_ADLER32 = 0, ALZ_CK_CRC32 = 1 } alz_checksum_kind;
int alz_checksum_batch(alz_ctx* ctx, uint32_t kind, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                       const alz_stream* ranges, uint32_t* out);
/* d_src_base is a DEVICE pointer; out is on the host */
int alz_checksum_batch_device(alz_ctx* ctx, uint32_t kind, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                              const alz_stream* ranges, uint32_t* out);
uint32_t alz_checksum_combine(uint32_t kind, uint32_t a, uint32_t b, uint64_t len_b);

/* ---------------------------------------- CRC-32C of byte ranges on the GPU
 * out[i] is the CRC-32C (Castagnoli: polynomial 0x82F63B78 reflected, start value and final inversion 0xFFFFFFFF; "123456789" gives
 * 0xE3069283) of the n ranges[i]: the checksum a framed Snappy file carries per chunk, BEFORE Snappy's mask (CRC32c.cs, Snappy.cs:252).
 * It is not a kind of alz_checksum_batch (whose kinds end at ALZ_CK_CRC32) but the same two launches over the other polynomial, and
 * everything said there holds: a range is src_off / src_len of its alz_stream, every other field is ignored; ranges may overlap, be
 * empty (0) and start at any byte; aligned 16-byte granules that each hold a byte of a range, so the 64-byte slack rule covers the
 * reads; one wavefront per 32 KiB chunk, one fold wavefront per range; alz_last_kernel_ms reports the device time of the two launches;
 * n == 0 is ALZ_OK; a NULL ctx, a range outside src_bytes, or NULL ranges / out with n > 0 are ALZ_E_INVALID; more than 2^31 chunks
 * are ALZ_E_UNSUPPORTED.  alz_crc32c_combine: the CRC-32C of A || B from those of A and B and the length of B; pure host code, the
 * arithmetic of the second launch; len_b == 0 returns a.  MI355X (docs/EXPERIMENTS.md 19): 10 000 ranges of 64 KiB at 952 GB/s, one
 * range of 64 MiB at 306 GB/s (one host thread with the SSE4.2 instruction: 10 - 13 GB/s). */
int alz_crc32c_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out);
/* d_src_base is a DEVICE pointer; out is on the host */
int alz_crc32c_batch_device(alz_ctx* ctx, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out);
uint32_t alz_crc32c_combine(uint32_t a, uint32_t b, uint64_t len_b);

/* ---------------------------------------- ZLib and GZip files in batches
 * What alz_zlib_decompress / alz_gzip_decompress (and their _measure twins) do for one file, for n files in one call.  files[i].format is
 * ALZ_ZFILE_ZLIB or ALZ_ZFILE_GZIP -- a batch may mix them, any other value is ALZ_E_INVALID; src_off / src_len is the whole file;
 * dst_off / dst_cap is where its output goes (measure: dst_off is ignored, dst_cap is the size limit); decom_len, aux0 and aux1 are
 * IGNORED.  All buffers are in host memory.
 * THE CONTRACT IS DIFFERENTIAL: results[i].rc / status / dst_len / src_used are exactly what the single-file call returns for file i
 * alone with the same capacity, and the bytes at [dst_off, dst_off + dst_len) are the bytes it delivers -- also for a file that fails
 * (its partial output is delivered).  Nothing outside a file's [dst_off, dst_off + dst_cap) is written.  A file's failure is that
 * file's rc; the call itself fails only for bad arguments or a HIP error.
 * One batch: the header walks run on the host (the code of the single-file layer); the source is uploaded once; all bodies decode as ONE
 * alz_inflate_decode_batch_device (measure: one measure batch); all outputs are summed in HBM by alz_checksum_batch_device, Adler-32 for
 * the ZLib files and CRC-32 for the GZip members (measure: taken as correct); the trailers are compared on the host; the outputs are
 * downloaded once.  A GZip member behind the first is found only when the one before it is decoded, so a batch runs in rounds: round r
 * holds the r-th member of every file that has one, each member with a CRC-32 and ISIZE check of its own.
 * NOT BUILT: device-resident forms (headers and trailers are read on the host), preset
 *   dictionaries.  The single-file entry points above are unchanged, host-side checksums included: they are the yardstick. */
#define ALZ_ZFILE_ZLIB 0u
#define ALZ_ZFILE_GZIP 1u
typedef struct alz_file_result {
    int32_t  rc;         /* ALZ_OK or the ALZ_E_* code of this file */
    int32_t  status;     /* alz_status (meaningful with ALZ_E_STREAM) */
    uint32_t dst_len;
    uint32_t src_used;
} alz_file_result;
int alz_zfile_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                           uint8_t* dst_base, size_t dst_bytes, alz_file_result* results);
int alz_zfile_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                            alz_file_result* results);

/* ---------------------------------------- DEFLATE written on the GPU: raw streams, ZLib and GZip files
 * The reference hands ZLib.Compress / GZip.Compress to the BCL (ZLib.cs:36-46, GZip.cs:36-43): its contract is "whatever the zlib behind
 * the BCL writes", any RFC 1951 stream that inflates back to the input.  BIT-IDENTITY DOES NOT APPLY HERE; the bar is the one of the
 * decoder read backwards: a stream is right when zlib's `inflate` (window bits -15) reads it to its end, with no byte left over and the
 * input as output, and alz_inflate_decode_batch reads it the same way.  So no code set is incomplete other than a single 1-bit code,
 * symbols 286 / 287 / 30 / 31 are never used, no distance exceeds 32 768 or reaches in front of the stream's start, no length exceeds
 * 258, no stored block holds more than 65 535 bytes.
 * alz_stream and alz_result are reused: src_off / src_len is the raw input, dst_off / dst_cap where the stream goes; decom_len, aux0, aux1
 * and format are IGNORED.  The slack rules are those of alz_inflate_*.  The kernels read nothing outside a stream's source range.
 * level    0..9 with zlib's meaning; 0 writes stored blocks only.  1..9 search harder as they rise -- per position the finder compares at
 *          most `chain` candidates of its hash chain, stops at a match of `nice` bytes, and from level 4 on parses lazily (a position
 *          whose successor has a longer match becomes a literal):
 *            level   1    2    3    4    5    6    7    8     9
 *            chain   4    8   16   16   32   64  128  256  1024
 *            nice   32   64  128  128  258  258  258  258   258
 *            lazy    -    -    -  yes  yes  yes  yes  yes   yes
 *          A match of 3 bytes further than 4 096 back is dropped (it costs more than its literals), as zlib does.
 * flags    ALZ_DEFLATE_FIXED: fixed Huffman codes only (what ZLib.cs:43 maps CompatibilityMode to).  Any other level or flag bit is
 *          ALZ_E_INVALID.
 * blocks   A stream is cut into blocks of alz_deflate_block_bytes() (32 704) input bytes; every kernel's unit of work is a block, so ONE
 *          long stream fills the GPU as a batch of short ones does.  A block's matches reach back into earlier blocks of its stream (the
 *          history is the input: a block first inserts the 32 KiB in front of it into its hash table).  Per block the encoder writes the
 *          smallest of the stored, the fixed and the dynamic form (with ALZ_DEFLATE_FIXED: of stored and fixed); the tokens of a block do
 *          not depend on `flags`, so the default is never larger than fixed-only.  Code lengths are limited to 15 (the code-length code:
 *          7) and every code set is complete, or a single 1-bit code; a block without a match has an empty distance set.
 *          BLOCKS MEET ON BYTE BOUNDARIES: a block that is neither stored nor the stream's last is followed by an EMPTY STORED BLOCK (3
 *          header bits, padding, 00 00 FF FF -- zlib's Z_SYNC_FLUSH), 4 to 5 bytes per block; in return no block waits for the
 *          bits in front of it.
 * results  OK: { ALZ_ST_OK, dst_len = bytes written, src_used = src_len }.  A stream that does not fit dst_cap: ALZ_ST_OUTPUT_CAPACITY
 *          with dst_len 0, as alz_rlh_encode_batch; nothing of it is written.  Nothing outside [dst_off, dst_off + dst_cap) is ever
 *          written.  alz_deflate_bound(n) = n + 5 per block always suffices (<= n + (n >> 10) + 64).  Empty input gives a valid stream of
 *          one final block.  Inputs of 0x7FFFFF00 bytes and more are ALZ_E_UNSUPPORTED.  n == 0 is ALZ_OK.
 * The output of a stream is a pure function of (bytes, level, flags): not of the batch around it, its alignment, the host or device form
 * or the context mode -- there is ONE set of kernels, as for inflate.  alz_last_kernel_ms reports the device time of the call's launches.
 *
 * The file layer.  kind is ALZ_ZFILE_ZLIB or ALZ_ZFILE_GZIP (anything else: ALZ_E_INVALID).
 *   zlib   78 01 / 78 5E / 78 9C / 78 DA for levels 0-1 / 2-5 / 6 / 7-9 (what zlib writes), the body, the big-endian Adler-32 of the input.
 *   gzip   1F 8B 08 00, MTIME 0, XFL (04 at levels 0-1, 02 at level 9, 00 otherwise), OS 03, the body, CRC-32 and ISIZE (src_len mod
 *          2^32), little-endian.
 * alz_deflate_file_compress stages the input once, runs the body as one alz_deflate_encode_batch_device of one stream and takes the
 *   checksum on the host; a dst_cap that is too small is ALZ_E_NOMEM (*dst_len is then 0); alz_deflate_file_bound(kind, n) suffices.
 * alz_deflate_file_compress_batch has the contract of alz_framing_compress_batch with files[i].format as the kind: DIFFERENTIAL against
 *   the single-file call on file i alone -- results[i] is { ALZ_OK, ALZ_ST_OK, dst_len, src_len } and the same bytes, or { that call's
 *   code, ALZ_ST_OK, 0, 0 }; one file's failure is that file's rc, and nothing outside a file's slot is written.  One batch: one upload,
 *   ONE alz_deflate_encode_batch_device over all bodies, one alz_checksum_batch_device per kind present over the raw inputs where they
 *   lie, the images assembled in HBM by one range copy, one download.
 * NOT BUILT: bit-exact concatenation of blocks, preset dictionaries, device-resident file forms. */
#define ALZ_DEFLATE_FIXED 1u
size_t alz_deflate_bound(size_t src_len);
int alz_deflate_block_bytes(void);
int alz_deflate_encode_batch(alz_ctx* ctx, int level, uint32_t flags, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                             const alz_stream* streams, uint8_t* dst_base, size_t dst_bytes, alz_result* results);
/* d_src_base / d_dst_base are DEVICE pointers; results come back to the host */
int alz_deflate_encode_batch_device(alz_ctx* ctx, int level, uint32_t flags, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                                    const alz_stream* streams, uint8_t* d_dst_base, size_t dst_bytes, alz_result* results);
size_t alz_deflate_file_bound(uint32_t kind, size_t src_len);
int alz_deflate_file_compress(alz_ctx* ctx, uint32_t kind, int level, uint32_t flags, const uint8_t* src, size_t src_len,
                              uint8_t* dst, size_t dst_cap, size_t* dst_len);
int alz_deflate_file_compress_batch(alz_ctx* ctx, int level, uint32_t flags, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                    const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results);

/* ---------------------------------------- XXH32 of byte ranges on the GPU
 * out[i] is XXH32 (xxHash, 32 bits: the block and content checksum of the LZ4 frame format, LZ4.Frame.cs:17-18) of the n ranges[i] with
 * `seed` (the frame format uses 0).  The argument rules are those of alz_checksum_batch*: a range is src_off / src_len of its alz_stream,
 * EVERY OTHER FIELD IS IGNORED; ranges may overlap, be empty (0x02CC5D05 with seed 0) and start at any byte; n == 0 is ALZ_OK; a NULL
 * ctx, a range outside src_bytes, or NULL ranges / out with n > 0 are ALZ_E_INVALID (checked before anything is uploaded).  The device
 * writes nothing but the n results (and the library's own scratch).  The kernel READS a range in aligned dwords, each of which holds a
 * byte of the range, so the slack rule of alz_aplib_* (64 readable bytes behind the buffer) covers it.
 * XXH32 is not linear -- the partial results of two pieces cannot be joined -- so one range is a serial chain over its 16-byte stripes:
 * four lanes work on a range (one per accumulator), 16 ranges share a wavefront, one launch.  The parallelism is the NUMBER of ranges:
 * thousands of frames of some KiB each are what this is for; one range of many MiB runs on four lanes and is better hashed on the host
 * (MI355X, docs/EXPERIMENTS.md 18: 10 000 ranges of 256 KiB at 742 GB/s; ONE range of 64 MiB at 0.33 GB/s, 42 x slower than one host
 * thread).  alz_last_kernel_ms reports the device time of the launch. */
int alz_xxh32_batch(alz_ctx* ctx, uint32_t seed, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                    const alz_stream* ranges, uint32_t* out);
/* d_src_base is a DEVICE pointer; out is on the host */
int alz_xxh32_batch_device(alz_ctx* ctx, uint32_t seed, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                           const alz_stream* ranges, uint32_t* out);

/* ---------------------------------------- LZ4 and Snappy files in batches
 * What alz_container_decompress / alz_container_measure do for one file of ALZ_C_LZ4_FRAME, ALZ_C_LZ4_LEGACY or ALZ_C_SNAPPY, for n files
 * in one call.  files[i].format is one of these three alz_container values -- a batch may mix them, any other value is ALZ_E_INVALID;
 * src_off / src_len is the whole file; dst_off / dst_cap is where its output goes (measure: dst_off is ignored, dst_cap is the size
 * limit); decom_len, aux0 and aux1 are IGNORED.  All buffers are in host memory.  alz_file_result is the one of alz_zfile_*.
 * THE CONTRACT IS DIFFERENTIAL, against the single-file call on file i alone with the same capacity (measure: the same limit):
 *   that call returns ALZ_OK or ALZ_E_STREAM:  results[i].rc / status / dst_len / src_used are what it returns, and the bytes at
 *     [dst_off, dst_off + dst_len) are the bytes it delivers -- also the partial output of a file that fails.
 *   it returns ALZ_E_FORMAT, ALZ_E_CHECKSUM or ALZ_E_UNSUPPORTED:  results[i].rc is that code, status is ALZ_ST_OK, dst_len and src_used
 *     are 0 and the bytes of the slot are unspecified (the single-file call leaves its out-parameters unset).
 * Nothing outside a file's [dst_off, dst_off + dst_cap) is written on the host.  A file's failure is that file's rc; the call itself fails
 * only for bad arguments or a HIP error.
 * One decode batch: the framing is read on the host by the readers of the single-file layer (block checksums are verified there, over
 * source bytes in host memory); the source is uploaded once and one device destination covers all slots.  The compressed LZ4 blocks of ALL
 * files are measured first (one alz_measure_batch_device), which settles every block's place; then a round is ONE device-resident decode:
 * the first holds every LZ4 block that reaches into nothing in front of itself -- of whatever frame or file -- and every compressed Snappy
 * chunk at its declared place; a block of a linked frame that reads earlier output runs one round behind the blocks in front of it, and
 * a Snappy file with a chunk that decodes to more than it declares is read on in order, one chunk per round.  Stored blocks and chunks
 * are copied HBM to HBM, one launch per round; the outputs of the frames with a content checksum are hashed where they lie by ONE
 * alz_xxh32_batch_device; the outputs are downloaded once.  alz_framed_measure_batch is the same walk without the decode, with content
 * checksums taken as correct and the declared content size checked.  MI355X (docs/EXPERIMENTS.md 18): 2 000 files of 64 KiB in one
 * call take 30 ms (LZ4 frames with content checksums) and 27 ms (Snappy), 11.7 and 10.4 times less than a loop of the single-file call.
 * NOT BUILT: device-resident forms, a second XXH32 layout for few long ranges, checksums fused into the kernels.  The single-file entry
 *   points are unchanged, host-side XXH32 included: they are the yardstick.  The write direction is alz_framing_compress_batch below. */
int alz_framed_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                            uint8_t* dst_base, size_t dst_bytes, alz_file_result* results);
int alz_framed_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                             alz_file_result* results);

/* ---------------------------------------- LZ4 and Snappy files WRITTEN in batches
 * What alz_container_compress does for one file of ALZ_C_LZ4_FRAME, ALZ_C_LZ4_LEGACY or ALZ_C_SNAPPY, for n files in one call.
 * files[i].format is one of these three alz_container values -- a batch may mix them, any other value makes the call ALZ_E_INVALID;
 * src_off / src_len is the raw input; dst_off / dst_cap is where the file goes; aux0 is the block size of an LZ4 frame (0, 0x10000,
 * 0x40000, 0x100000 or 0x400000: what alz_container_options.chunk_size is for the single-file call; the other two containers ignore it);
 * decom_len and aux1 are IGNORED.  One `settings` applies to the whole call; NULL is quality 8.  All buffers are in host memory.
 * THE CONTRACT IS DIFFERENTIAL, against alz_container_compress on file i alone with the same context, settings, block size and capacity:
 *   that call returns ALZ_OK:  results[i] is { ALZ_OK, ALZ_ST_OK, dst_len, src_len } and the dst_len bytes at dst_off are the bytes it writes.
 *   it returns another code:   results[i] is { that code, ALZ_ST_OK, 0, 0 } and the bytes of the slot are unspecified -- ALZ_E_NOMEM for
 *     a slot that is too small (also below the writers' floors: 16 bytes for LZ4, 10 for Snappy), ALZ_E_INVALID for an LZ4 input whose
 *     last block would hold 1 to 4 bytes (LZ4.cs:208 throws) and for an aux0 the frame format does not have.
 * Nothing outside a file's [dst_off, dst_off + dst_cap) is written on the host; one file's failure never changes another file's result.
 * The call itself fails only for bad arguments (a NULL ctx; n > 0 with NULL pointers; a range outside src_bytes / dst_bytes; settings
 * the encoder refuses) or a HIP error.  n == 0 is ALZ_OK.
 * One batch: the host lays out every block of every file the writer does not refuse beforehand (64 KiB chunks for Snappy, aux0 for
 * frames, 8 MiB for legacy); the source is uploaded once; all blocks of all files are ONE alz_encode_batch_device (LZ4 blocks and raw
 * Snappy chunks mix: one launch sequence per format), each into a slot of the size the single-file writer gives it; the raw bytes of
 * all Snappy chunks are hashed where they lie by ONE alz_crc32c_batch_device; the writers of the single-file layer (csrc/alz_framing.h)
 * then settle per file what is stored and what compressed, the size words and masked CRCs, the length and the verdict against dst_cap;
 * the file images are assembled in HBM by ONE range copy out of slots, source and a small uploaded table of header bytes, and
 * downloaded once.  A batch whose source plus slots exceed 2 GiB runs as consecutive groups of whole files (a larger file alone); the
 * results do not depend on the grouping.  A small legacy file or default-size frame still occupies the slot of a full block.
 * MI355X (docs/EXPERIMENTS.md 19): 2 000 inputs of 64 KiB in one call take 29 - 44 ms (LZ4 frames and Snappy, quality 0 and 8), 9.5 to
 * 16 times less than a loop of the single-file call; most of what is left is the download of the slots.
 * NOT BUILT: device-resident forms, frames with checksums or a content size (the reference's writer clears those flags,
 *   LZ4.Frame.cs:184), linked blocks.  The single-file entry point is unchanged, host-side CRC-32C included: it is the yardstick. */
int alz_framing_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                               const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results);

/* -------------------------------------------- decode: device-resident batches
 * The measured path: payload already in HBM, output left in HBM.  The kernels never WRITE outside a stream's
 * [dst_off, dst_off + dst_len) (tests/test_gpu_canary.py); they READ the input in aligned 16-byte granules and, for the 64 KiB
 * formats, up to 24 bytes beyond a source position of the stream's own output, so both device buffers need 64 readable bytes
 * behind the end of their last stream -- alz_device_malloc adds that slack to every allocation by itself.
 * alz_plan_create uploads the descriptor table and groups it per format (one
 * kernel launch per format present).  alz_plan_execute only enqueues kernels
 * on `hip_stream` (a hipStream_t, or NULL for the context's own stream) and
 * does not synchronise.  d_src_base / d_dst_base are DEVICE pointers.
 * One plan may be executed again while an earlier execute is still in flight, also on another stream and into other buffers.  Two kinds of plan own MUTABLE state on the
 * device -- a plan of big streams (the whole-GPU path, alz_ctx_big_stream: its scratch) and a plan that runs a format as a work queue of chunks (alz_ctx_set_kernel_variant:
 * queue heads, hand-over flags and slots) -- so their executes are ordered one behind the other by an event, whichever streams they are enqueued on (they do not
 * overlap; a caller who wants two batches in flight creates two plans); any other plan only reads its tables.  Every plan has ONE result table: alz_plan_results
 * returns the results of the LAST execute and waits for it, whichever stream it was enqueued on. */
int  alz_plan_create(alz_ctx* ctx, const alz_lz_properties* props, uint32_t n,
                     const alz_stream* streams, alz_plan** out);
int  alz_plan_execute(alz_ctx* ctx, alz_plan* plan, const void* d_src_base, void* d_dst_base, void* hip_stream);
/* Runs `iters` executions bracketed by HIP events on the launch stream and returns the
 * mean milliseconds per execution (kernel time as seen by the device). Synchronises. */
int  alz_plan_execute_timed(alz_ctx* ctx, alz_plan* plan, const void* d_src_base, void* d_dst_base,
                            int iters, float* mean_ms);
int  alz_plan_results(alz_ctx* ctx, alz_plan* plan, alz_result* results); /* synchronises, copies n results */
void alz_plan_destroy(alz_ctx* ctx, alz_plan* plan);

/* The device-resident path over several contexts = several GPUs of one node, without host staging: what
 * alz_decode_batch_multi does for host buffers, for a caller whose compressed payload is already in HBM (and whose output stays there).
 * alz_plan_create_multi partitions the batch (part_of[i] = index into ctxs[] that decodes stream i; NULL: alz_partition_batch decides,
 * part_of_out -- may be NULL -- receives the choice) and creates one plan per context over that context's streams.  A stream's
 * src_off / dst_off are relative to the device pointers of ITS context: d_src_bases[q] / d_dst_bases[q] in alz_plan_execute_multi, which
 * only enqueues every context's kernels on that context's own stream (from the calling thread: launches are asynchronous, no host
 * threads, no collective -- streams are independent, a fresh LzWindows per Decompress call, Nintendo/LZ10.cs:86) and does not
 * synchronise.  alz_plan_results_multi waits for all of them and returns the n results in batch order.  ctxs[] must not repeat a
 * context; two contexts may share a device. */
typedef struct alz_multi_plan alz_multi_plan;
int  alz_plan_create_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, uint32_t n,
                           const alz_stream* streams, const uint32_t* part_of, alz_multi_plan** out, uint32_t* part_of_out);
int  alz_plan_execute_multi(alz_multi_plan* plan, const void* const* d_src_bases, void* const* d_dst_bases);
int  alz_plan_results_multi(alz_multi_plan* plan, alz_result* results);
void alz_plan_destroy_multi(alz_multi_plan* plan);

/* ------------------------------------------------------------- encode
 * Replaces the static `CompressHeaderless(ReadOnlySpan<byte>, Stream, CompressionSettings)`
 * bodies (e.g. LZSS.cs:132-160, LZ10.cs:113-137) + LzChainMatchFinder
 * (src/AuroraLib.Compression/MatchFinder/LzChainMatchFinder.cs:157-212).
 * For encode, alz_stream.src_* describe the RAW input and dst_* the compressed
 * output capacity; results[i].dst_len is the compressed size.  For YAY0/MIO0
 * the three sections are written flags|tokens|literals and aux0/aux1 of the
 * result are returned in alz_encode_aux. */
typedef struct alz_encode_aux { uint32_t aux0; uint32_t aux1; } alz_encode_aux;
int alz_encode_batch(alz_ctx* ctx, const alz_lz_properties* props, const alz_settings* settings, uint32_t n,
                     const uint8_t* src_base, size_t src_bytes,
                     const alz_stream* streams,
                     uint8_t* dst_base, size_t dst_bytes,
                     alz_result* results, alz_encode_aux* aux /* may be NULL */);

/* The same with the raw buffers already in HBM and the compressed streams left there: alz_stream.src_off / dst_off are
 * relative to the two DEVICE pointers.  What a caller that produces its input on the device uses, and what bench.py times
 * (kernels, no PCIe); alz_last_kernel_ms() reports the device time of the call.  Nothing outside [d_src_base, d_src_base +
 * src_bytes) is read and nothing outside a stream's [dst_off, dst_off + dst_cap) is written: the finder's look-ahead loads run up
 * to 32 bytes past a stream's end, so a stream that ends inside the last 64 bytes of the source buffer is searched in a scratch copy. */
int alz_encode_batch_device(alz_ctx* ctx, const alz_lz_properties* props, const alz_settings* settings, uint32_t n,
                            const void* d_src_base, size_t src_bytes,
                            const alz_stream* streams,
                            void* d_dst_base, size_t dst_bytes,
                            alz_result* results, alz_encode_aux* aux /* may be NULL */);
/* alz_encode_batch over several contexts (one per GPU), as alz_decode_batch_multi: every CompressHeaderless call builds its own
 * LzChainMatchFinder (src/AuroraLib.Compression/Formats/Common/LZSS.cs:135), so the buffers of a batch are independent; the
 * library deals them out by raw size (longest first onto the least loaded context), every context receives and returns only
 * its share, one host thread per context, no collective.  part_of_out (may be NULL): the context each stream ran on.  The
 * output is byte-identical to alz_encode_batch on one context. */
int alz_encode_batch_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, const alz_settings* settings, uint32_t n,
                           const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results, alz_encode_aux* aux /* may be NULL */,
                           uint32_t* part_of_out /* may be NULL */);

/* ------------------------------------------------ device memory helpers
 * For hosts without their own HIP allocator (the C# shim, the test harness). */
int alz_device_malloc(alz_ctx* ctx, size_t bytes, void** d_ptr);
int alz_device_free(alz_ctx* ctx, void* d_ptr);
int alz_memcpy_h2d(alz_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int alz_memcpy_d2h(alz_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int alz_memset_d(alz_ctx* ctx, void* d_dst, int value, size_t bytes);
int alz_synchronize(alz_ctx* ctx);
/* Measurement helper ("achievable copy bandwidth as a second denominator"): a 16 B/lane device-to-device copy
 * kernel over `bytes`, `iters` times; *gb_per_s = (bytes read + bytes written) / time. */
int alz_measure_copy_bandwidth(alz_ctx* ctx, size_t bytes, int iters, double* gb_per_s);
/* Device time (HIP events on the launch stream) of the kernels of the last alz_plan_execute_timed (mean per execution) or
 * alz_encode_batch (hash-table resets + all encode kernels of the call) on this context. */
int alz_last_kernel_ms(alz_ctx* ctx, float* ms);

/* ------------------------------------------------ container layer (host side)
 * The managed part of the reference's format classes restated above the
 * ABI: header parse/emit + endianness retry, body on the GPU.  One function
 * per ICompressionAlgorithm member.  `container` values are alz_container. */
typedef enum alz_container {
    ALZ_C_LZSS   = 0,  /* "LZSS"+BE size+BE csize+0      LZSS.cs:53-88   */
    ALZ_C_LZ10   = 1,  /* 0x10 + u24 LE size             LZ10.cs:47-80   */
    ALZ_C_LZ11   = 2,  /* 0x11 + u24 LE size             LZ11.cs:43-81   */
    ALZ_C_YAZ0   = 3,  /* "Yaz0"+size+align+0            Yaz0.cs:58-88   */
    ALZ_C_YAY0   = 4,  /* "Yay0"+size+tokOff+litOff      Yay0.cs:50-77   */
    ALZ_C_MIO0   = 5,  /* "MIO0"+size+tokOff+litOff      MIO0.cs:51-79   */
    ALZ_C_PRS    = 6,  /* headerless                     PRS.cs:38-57    */
    ALZ_C_LZ4_LEGACY = 7, /* LZ4Legacy: 0x184C2102 + u32-sized independent 8 MiB blocks + 0xFF   LZ4Legacy.cs, LZ4.cs:96-111,120-135 */
    ALZ_C_LZO    = 8,  /* headerless                     LZO.cs:42-47    */
    ALZ_C_SNAPPY = 9,  /* framed "sNaPpY": 64 KiB chunks (one GPU batch) + masked CRC-32C   Snappy.cs:39-107 */
    /* header-only wrappers over the same bodies */
    ALZ_C_GCLZ   = 10, /* "GCLZ" + LZ10 file             src/AuroraLib.Compression.Nintendo/Nintendo/GCLZ.cs        */
    ALZ_C_CXLZ   = 11, /* "CXLZ" + LZ10 file             src/AuroraLib.Compression.Nintendo/Sega/CXLZ.cs            */
    ALZ_C_LZ_3DS = 12, /* "3DS-LZ\r\n" + LZ10 file       src/AuroraLib.Compression.Nintendo/Nintendo/3DS-LZ.cs      */
    ALZ_C_COMP   = 13, /* "COMP" + LZ11 file             src/AuroraLib.Compression.Nintendo/Sega/COMP.cs            */
    ALZ_C_YAZ1   = 14, /* Yaz0 with magic "Yaz1"         src/AuroraLib.Compression.Nintendo/Nintendo/Yaz1.cs        */
    ALZ_C_AKLZ   = 15, /* 12-byte magic + BE size + LZSS src/AuroraLib.Compression.Sega/Sega/AKLZ.cs:41-56          */
    ALZ_C_LZ01   = 16, /* "LZ01"+csize+size+0 + LZSS     src/AuroraLib.Compression.Sega/Sega/LZ01.cs:47-83          */
    ALZ_C_LZSEGA = 17, /* csize+size + LZSS              src/AuroraLib.Compression.Sega/Sega/LZSega.cs:49-68        */
    ALZ_C_LEVEL5LZSS = 18, /* "SSZL"+0+csize+size + LZSS src/AuroraLib.Compression.Nintendo/Level5/Level5LZSS.cs:42-72 */
    ALZ_C_LZON   = 19, /* "LZOn"+002FF171+BE size+csize + LZO  src/AuroraLib.Compression.Nintendo/Nintendo/LZOn.cs:41-79 */
    ALZ_C_LZ77   = 20, /* "LZ77"+type: LZ10 / LZ11 / ChunkLZ10 (independent 4 KiB chunks = one GPU batch) / RLE30 / HUF20  Nintendo/LZ77.cs:56-153 */
    ALZ_C_LEVEL5 = 21, /* u32 type|size<<3: OnlySave / LZ10 / Huffman4Bit / Huffman8Bit / RLE   src/AuroraLib.Compression.Nintendo/Level5/Level5.cs:62-146 */
    ALZ_C_LZ4_FRAME = 22, /* LZ4: frame 0x184D2204 (descriptor, linked or independent blocks, xxHash32 block / content
                             checksums), legacy and skippable frames, concatenated   LZ4.cs:50-93, LZ4.Frame.cs:107-215.
                             Decoding: a frame none of whose blocks reaches in front of itself (a host walk over the sequences)
                             is ONE GPU batch whatever its block-independence flag says -- the reference's own writer clears
                             the flag and compresses every block on its own --; any other frame decodes block after block */
    /* more header-only wrappers (the reference's .Extended assembly) */
    ALZ_C_MDB4   = 23, /* "MDB4"+(n+1)+n+csize+16 zero bytes + LZSS   src/AuroraLib.Compression-Extended/Specialized/MDB4.cs:33-72 */
    ALZ_C_FCMP   = 24, /* "FCMP"+n+0x12340000 + LZSS               src/AuroraLib.Compression-Extended/Marvelous/FCMP.cs:36-50    */
    ALZ_C_IECP   = 25, /* "IECP"+n + LZSS                          src/AuroraLib.Compression-Extended/Marvelous/IECP.cs:35-46    */
    ALZ_C_GCZ    = 26, /* n + LZSS (recognised by file extension only: IsMatch is always 0 here)   Konami/GCZ.cs:23-42          */
    ALZ_C_ECD    = 27, /* "ECD"+flag+BE plain/csize/size; 4 plain bytes + LZSS(10,6,2), or stored   Specialized/ECD.cs:45-109   */
    ALZ_C_SDPC   = 28, /* "SDPC"+n + LZO                           src/AuroraLib.Compression-Extended/Specialized/SDPC.cs:34-54 */
    ALZ_C_LZ40   = 29, /* 0x40 + u24 LE size + LZ40 body (negated MSB-first flag bytes, LE tokens)   Nintendo/LZ40.cs:40-77 */
    ALZ_C_LZ60   = 30, /* 0x60 + u24 LE size + the same body                                         Nintendo/LZ60.cs:29-58 */
    ALZ_C_LZHUDSON = 31, /* BE size + LZHudson body                 src/AuroraLib.Compression.Nintendo/HudsonSoft/LZHudson.cs:33-51 */
    ALZ_C_SMSR00 = 32, /* "SMSR00"+u16 0+BE size+BE literal pointer + codes | literals   Nintendo/SMSR00.cs:41-66 */
    ALZ_C_LZ00   = 33, /* "LZ00"+csize+8x0+name[32]+size+key+8x0, then an LZSS body XORed with the keystream of `key`
                          src/AuroraLib.Compression.Sega/Sega/LZ00.cs:40-96, :128-141 (see alz_container_options.key) */
    ALZ_C_FASTLZ = 34, /* headerless FastLZ stream, levels 1 / 2 (IsMatch = FastLZ.Validate; written at level 1)
                          src/AuroraLib.Compression/Formats/Common/FastLZ.cs:29-52, :246-291 */
    ALZ_C_BLZ    = 36, /* code section (stored back to front) + 0xFF padding + u24 LE total size + header size + i32 LE size delta
                          src/AuroraLib.Compression.Nintendo/Nintendo/BLZ.cs:28-95 */
    ALZ_C_CLZ0   = 37, /* "CLZ\0" + BE size + BE 0 + BE size + CLZ0 body   src/AuroraLib.Compression-Extended/Marvelous/CLZ0.cs:41-62 */
    ALZ_C_CNS    = 38, /* "@CNS" + extension[4] + LE size + 0 + CNS body   src/AuroraLib.Compression-Extended/Specialized/CNS.cs:44-75 */
    ALZ_C_LZ02   = 39, /* type byte (1 / 2) + u24 BE size + LZ02 body [+ extension data]   src/AuroraLib.Compression-Extended/Camelot/LZ02.cs:60-75 */
    ALZ_C_REFPACK = 40, /* [u32 LE compressed size] + flags + 0xFB + BE u24/u32 size [+ compressed size] + RefPack body; written with
                          the pre-header (version 2)   src/AuroraLib.Compression-Extended/EA/RefPack.cs:38-175 */
    ALZ_C_WFLZ   = 41, /* "WFLZ" + compressed size + size (FormatByteOrder, default little) + WFLZ body
                          src/AuroraLib.Compression-Extended/WayForward/WFLZ.cs:36-105 */
    ALZ_C_LZSHREK = 42, /* u32 LE 0x10 + size + compressed size + 0 + LZShrek body   src/AuroraLib.Compression-Extended/Activision/LZShrek.cs:22-71 */
    ALZ_C_HIG    = 43, /* "HIG!" + 15 ints (data offset, ..., version, size) [+ compressed size + path[0x7C] for versions 5 / 6] + HIG body
                          src/AuroraLib.Compression-Extended/Specialized/HIG.cs:47-124 */
    ALZ_C_CNX2   = 35, /* "CNX\x02" + extension[4] + BE csize + BE size + CNX2 body   src/AuroraLib.Compression.Sega/Sega/CNX2.cs:45-81 */
    /* the non-LZ bodies of the GBA / DS family (alz_rlh_*): a header of type + u24 LE size, or type + u24 0 + u32 LE size */
    ALZ_C_RLE30  = 44, /* 0x30 + size + RLE30 body                        src/AuroraLib.Compression.Nintendo/Nintendo/RLE30.cs:29-74 */
    ALZ_C_HUF20  = 45, /* 0x24 / 0x28 + size + HUF20 body (little nibble order); decode only   Nintendo/HUF20.cs:46-92 */
    ALZ_C_COUNT  = 46
} alz_container;

/* alz_container_options.variant for ALZ_C_LZ77 (LZ77.CompressionType, LZ77.cs:156-164) and ALZ_C_LEVEL5 (Level5.cs:151-159) */
#define ALZ_LZ77_LZ10      0x10u
#define ALZ_LZ77_LZ11      0x11u
#define ALZ_LZ77_CHUNKLZ10 0xF7u
#define ALZ_LZ77_HUF20_4   0x24u   /* decode only (HUF20 has no encoder: see alz_rlh_format) */
#define ALZ_LZ77_HUF20_8   0x28u   /* decode only */
#define ALZ_LZ77_RLE30     0x30u
#define ALZ_LEVEL5_ONLYSAVE 0u
#define ALZ_LEVEL5_LZ10     1u
#define ALZ_LEVEL5_HUFFMAN4 2u     /* decode only; big nibble order (Level5.cs:94-105) */
#define ALZ_LEVEL5_HUFFMAN8 3u     /* decode only */
#define ALZ_LEVEL5_RLE      4u

typedef struct alz_container_options {
    uint32_t big_endian;          /* IEndianDependentFormat.FormatByteOrder: 1 = Endian.Big (default for Yaz0/Yay0/MIO0/PRS) */
    uint32_t memory_alignment;    /* Yaz0.MemoryAlignment (Yaz0.cs:39) */
    alz_lz_properties lz;         /* LZSS geometry */
    uint32_t variant;             /* LZ77.Type / Level5.Type / HUF20.Type (0x24 / 0x28) when compressing; 0 = the class default (LZ10) */
    uint32_t chunk_size;          /* LZ77.ChunkSize (default 0x1000); ALZ_C_LZ4_FRAME: LZ4.BlockSize, one of 0x10000 /
                                     0x40000 / 0x100000 / 0x400000 (0 = the class default Block4MB, LZ4.cs:33) */
    uint32_t key;                 /* ALZ_C_LZ00 when compressing: the keystream seed written to the header (LZ00.Compress(..., uint key, ...)
                                     LZ00.cs:71; the parameterless overload passes the Unix time) */
    uint8_t  name[32];            /* ALZ_C_LZ00 when compressing: LZ00.Name, zero padded (all zero = the class default "Temp.dat", LZ00.cs:30) */
} alz_container_options;

/* IProvidesDecompressedSize.GetDecompressedSize (Interfaces/IProvidesDecompressedSize.cs:20) */
int alz_container_decompressed_size(uint32_t container, const alz_container_options* opt,
                                    const uint8_t* src, size_t src_len, uint32_t* size_out);
/* IFormatInfoProvider.IsMatch (e.g. LZ10.cs:36-41): 1 match, 0 no match */
int alz_container_is_match(uint32_t container, const uint8_t* src, size_t src_len);
/* ICompressionDecoder.Decompress(Stream, Stream).  On ALZ_E_STREAM, *status holds the alz_status. */
int alz_container_decompress(alz_ctx* ctx, uint32_t container, const alz_container_options* opt,
                             const uint8_t* src, size_t src_len,
                             uint8_t* dst, size_t dst_cap, size_t* dst_len, size_t* src_used, int32_t* status);
/* Decompressed size of a file of a container WITHOUT a size field -- PRS, LZO, FASTLZ, LZ4_FRAME, LZ4_LEGACY, SNAPPY -- by
 * measuring its bodies on the GPU (alz_measure_batch: all blocks / chunks of the file as one batch, linked LZ4 blocks included).
 * The outcome is that of reading the file in order into a destination of size_limit bytes: rc, *status, *size_out (what
 * *dst_len would be) and *src_used -- with an LZ4 frame's CONTENT checksum taken as correct (it needs the bytes; block checksums
 * cover stored bytes and are verified), and a framed Snappy chunk whose body ends short of its declared length read on from
 * where the body stopped, as the managed reader does (alz_container_decompress refuses such a chunk with ALZ_E_FORMAT).
 * A size_limit below the true size gives ALZ_E_STREAM / ALZ_ST_OUTPUT_CAPACITY.  Other containers: ALZ_E_UNSUPPORTED (they
 * have alz_container_decompressed_size). */
int alz_container_measure(alz_ctx* ctx, uint32_t container, const alz_container_options* opt,
                          const uint8_t* src, size_t src_len, size_t size_limit,
                          size_t* size_out, size_t* src_used, int32_t* status);
/* ICompressionEncoder.Compress(ReadOnlySpan<byte>, Stream, CompressionSettings) */
int alz_container_compress(alz_ctx* ctx, uint32_t container, const alz_container_options* opt,
                           const alz_settings* settings,
                           const uint8_t* src, size_t src_len,
                           uint8_t* dst, size_t dst_cap, size_t* dst_len);
/* worst-case compressed size for dst_cap sizing */
size_t alz_container_compress_bound(uint32_t container, size_t src_len);

/* ---------------------------------------- the wrapped files: RLHudson and the seven wrapper classes of the .Extended assembly
 * Eight classes of the reference are a small header over a body the library already decodes.  They are no alz_container values (ALZ_C_COUNT
 * stays 46): one kind enum and entry points of their own.  Paths relative to src/AuroraLib.Compression-Extended.
 *   ALZ_WF_ASURAZLB  EA/AsuraZlb.cs       "AsuraZlb", u32 LE 1, u32 BE compressed size, u32 BE size, a BOUNDED zlib stream
 *   ALZ_WF_ZLB       Rare/ZLB.cs          "ZLB\0", u32 BE 1, u32 BE size, u32 BE compressed size, a BOUNDED zlib stream
 *   ALZ_WF_MDF0      Konami/MDF0.cs       "mdf\0", u32 LE size, a zlib stream to the end
 *   ALZ_WF_RAREZIP   Rare/RareZip.cs      11 72, u32 BE size, a RAW DEFLATE stream to the end
 *   ALZ_WF_HWGZ      Specialized/HWGZ.cs  chunk size, count, size (byte order detected: little first, then big), a table of count words that
 *                                         the reader never looks at, then, each aligned to 128 from the start of the file, count x (size word in
 *                                         FormatByteOrder = opt->big_endian whatever was detected, a BOUNDED zlib stream).  A batch inside one file.
 *   ALZ_WF_SSZL      Specialized/SSZL.cs  "SSZL", u32 LE 0x20101109, u32 LE size, u32 LE Options, u32 0, then the payload: XORed with a
 *                                         Mersenne-Twister keystream (seed 0x40C360F3) if Options & 0x80000000; a gzip file if Compressed (bit 0)
 *                                         and it starts 1F 8B, a zlib file to the end if Compressed, otherwise plain bytes.
 *   ALZ_WF_ZLWF      WayForward/ZLWF.cs   "ZLWF", compressed size, size, count, count offsets (FormatByteOrder), each the start of a whole WFLZ
 *                                         file (ALZ_C_WFLZ) of that byte order.  NOT a zlib wrapper.  A batch inside one file.
 *   ALZ_WF_RLHUDSON  src/AuroraLib.Compression.Nintendo/HudsonSoft/RLHudson.cs   u32 BE size, u32 BE 5, an RLHudson body (alz_rlhudson_*)
 * alz_wfile_is_match is each class's IsMatchStatic, statement for statement, odd length tests included (ZLB asks for more than 0x14 bytes
 * behind a 16-byte header; HWGZ for 0x80 bytes and ZLib.IsMatchStatic four bytes behind the aligned table; MDF0 tests the zlib header too).
 * alz_wfile_walk is pure host code and needs no context: it returns the file's parts {src_off, src_len, body, dst_len} (dst_len: the decoded
 * size a part states itself -- WFLZ, RLHudson -- else 0), the size the header states and, for SSZL, its Options in *flags; an encrypted SSZL part
 * is still encrypted where it lies.  cap too small: ALZ_E_INVALID with *n_parts = the count needed.  Wrong magic (an HWGZ header that validates in
 * neither order, a ZLWF chunk without "WFLZ"): ALZ_E_FORMAT.  A header, table or chunk that runs past the input -- an HWGZ count or chunk, a ZLWF
 * count or offset outside the file: ALZ_E_STREAM (INPUT_TRUNCATED).  A caller with device-resident data feeds the parts to the _device batch calls.
 * alz_wfile_decompress has the signature and conventions of alz_zlib_decompress; a NULL ctx is ALZ_E_INVALID only once a body must be decoded.
 * alz_wfile_decode_batch: files[i].format is the kind (a batch may mix them), aux0 bit 0 the file's FormatByteOrder (1 = big; HWGZ, ZLWF).  THE
 *   CONTRACT IS DIFFERENTIAL, as alz_zfile_decode_batch's: file i's result and bytes are exactly what alz_wfile_decompress returns for it
 *   alone with the same capacity; a file's failure is that file's rc.  The walks run on the host; the source goes to the device once (SSZL
 *   payloads XORed before, the keystream drawn once per call) and all parts of all files decode as one batch per body kind: one
 *   alz_inflate_decode_batch_device for every zlib and raw DEFLATE part with one alz_checksum_batch_device for the Adler-32s, one plan of WFLZ
 *   bodies, one alz_rlhudson_decode_batch_device.  A part's destination is the sum of the decoded sizes in front of it: an HWGZ file's chunks
 *   are MEASURED first (one alz_inflate_measure_batch_device; ChunkSize is a writer's convention that the reader never enforces), a ZLWF chunk
 *   states its size.  SSZL gzip payloads go through alz_zfile_decode_batch.
 * Rules where the reference leaves room:
 *   bounded zlib bodies (AsuraZlb, ZLB, each HWGZ chunk): the body is src[hdr, hdr + min(csize, bytes left)); result and bytes are
 *     alz_zlib_decompress's on that range, EXCEPT that a body whose DEFLATE data ended properly and whose trailer has fewer than 4 bytes inside
 *     the bound is ALZ_OK with the checksum unverified: the reference's own ZLB.Compress writes csize four short and its round-trip test passes
 *     such files.  (Nobody has run the BCL on such a file here.)  A full trailer is verified: ALZ_E_CHECKSUM, output delivered.
 *   stated sizes: AsuraZlb, ZLB, HWGZ, MDF0, SSZL, ZLWF: after an otherwise successful decode dst_len != stated is ALZ_E_STREAM /
 *     OUTPUT_SIZE_MISMATCH with the output delivered.  RareZip and RLHudson use the '>' rule only; a RareZip body that decodes to fewer bytes
 *     is ALZ_OK, the bytes up to the stated size are zero (SetLength) and dst_len is the stated size, limited by dst_cap.  A body that meets
 *     dst_cap first is OUTPUT_CAPACITY.  A ZLWF chunk decodes into the size its WFLZ header states and no further: a body that runs past it is
 *     OUTPUT_SIZE_MISMATCH with the stated bytes of that chunk delivered (dst_len ends there); one that ends short is the same status.  A ZLWF
 *     file of no chunks with a non-zero stated size is a mismatch too, alone or in any batch.
 * Writing.  RLHudson and ZLWF have managed bytes: alz_wfile_compress is bit-identical for them (level, flags ignored; ZLWF blocks through
 *   alz_container_compress(ALZ_C_WFLZ)).  The six DEFLATE kinds have none (the reference hands Compress to the BCL): settings is ignored, level /
 *   flags go to alz_deflate_*; all chunks of an HWGZ file are ONE alz_deflate_file_compress_batch; header fields as the reference's header code
 *   writes them, ZLB's compressed size four short included; the HWGZ table is written correctly in the file's order.  opt->chunk_size: HWGZ
 *   ChunkSize (0 = 0x10000), ZLWF BlockSize (0 = 0x400000); opt->variant: SSZL Options to write (0 = Compressed | Encrypted).
 * NOT BUILT: device-resident file forms, rows of alz_brute_force / alz_container_scan, shim classes, Brotli (RFC 7932's static dictionary). */
typedef enum alz_wfile_kind {
    ALZ_WF_ASURAZLB = 0, ALZ_WF_ZLB, ALZ_WF_MDF0, ALZ_WF_RAREZIP,
    ALZ_WF_HWGZ, ALZ_WF_SSZL, ALZ_WF_ZLWF, ALZ_WF_RLHUDSON, ALZ_WF_COUNT
} alz_wfile_kind;
typedef enum alz_wfile_body {
    ALZ_WB_ZLIB = 0, ALZ_WB_GZIP, ALZ_WB_DEFLATE, ALZ_WB_WFLZ, ALZ_WB_WFLZ_BE, ALZ_WB_RLHUDSON, ALZ_WB_PLAIN
} alz_wfile_body;
typedef struct alz_wfile_part { uint32_t src_off, src_len, body, dst_len; } alz_wfile_part;
#define ALZ_SSZL_COMPRESSED 0x1u
#define ALZ_SSZL_USE_GZIP   0x2u
#define ALZ_SSZL_ENCRYPTED  0x80000000u
int alz_wfile_is_match(uint32_t kind, const uint8_t* src, size_t len);
int alz_wfile_decompressed_size(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, uint32_t* size_out);
int alz_wfile_walk(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, alz_wfile_part* parts, uint32_t cap,
                   uint32_t* n_parts, uint32_t* stated_size, uint32_t* flags);
int alz_wfile_decompress(alz_ctx* ctx, uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len,
                         uint8_t* dst, size_t dst_cap, size_t* dst_len, size_t* src_used, int32_t* status);
int alz_wfile_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                           uint8_t* dst_base, size_t dst_bytes, alz_file_result* results);
size_t alz_wfile_compress_bound(uint32_t kind, const alz_container_options* opt, size_t src_len);
int alz_wfile_compress(alz_ctx* ctx, uint32_t kind, const alz_container_options* opt, const alz_settings* settings, int level, uint32_t flags,
                       const uint8_t* src, size_t len, uint8_t* dst, size_t dst_cap, size_t* dst_len);

/* ------------------------------------------------ batch producers
 * The two places in the reference that issue many independent decodes, restated as callers of the batched path.
 *
 * alz_container_scan: ScanDecompressCommand (src/AuroraLib.Compression.CLI/Commands/ScanDecompressCommand.cs:12-104).
 * Walks `src` byte by byte; at every offset the first container of `containers` whose IsMatch accepts identifies the
 * format (FormatService.Formats.Identify, :62); the stream is decoded and kept when it decodes without an exception
 * and yields more than 0x10 bytes (:85), the walk then continues behind it (:98), otherwise at the next byte (:100).
 * Here every candidate offset is decoded in ONE GPU batch (rounds of <= 1 GiB of output) and the walk is replayed over
 * the results.  Supported: the containers with a size header and one body (LZSS, LZ10, LZ11, YAZ0, YAY0, MIO0, GCLZ,
 * CXLZ, LZ_3DS, COMP, YAZ1, AKLZ, LZ01, LZSEGA, LEVEL5LZSS, MDB4, FCMP, IECP, LZ40, LZ60, CNX2, CLZ0, CNS, SMSR00, HIG).  A Yaz0 /
 * Yaz1 candidate that fails is decoded once more with its size field byte-swapped, as Yaz0.Decompress does (Yaz0.cs:66-78).
 * Outputs of the accepted streams are packed into dst in file order; ALZ_E_NOMEM when dst or hits is too small
 * (nhits / dst_used then describe what fitted). */
typedef struct alz_scan_hit {
    uint64_t start;      /* offset of the stream in src */
    uint64_t end;        /* source.Position after Decompress */
    uint64_t dst_off;    /* its output inside dst */
    uint32_t dst_len;
    uint32_t container;  /* alz_container that identified it */
} alz_scan_hit;
int alz_container_scan(alz_ctx* ctx, const uint32_t* containers, uint32_t n_containers, const alz_container_options* opt,
                       const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                       alz_scan_hit* hits, uint32_t max_hits, uint32_t* nhits, size_t* dst_used);

/* alz_brute_force: BruteForceCommand (src/AuroraLib.Compression.CLI/Commands/BruteForceCommand.cs:24-133): one raw
 * buffer, every raw decoder of the path tried against a fixed destination of `expected_size` bytes -- one GPU batch per
 * LZSS geometry.  Decoder i writes to dst + i * slot (slot >= expected_size); it "successfully unpacked the file" (:42)
 * when results[i].status == ALZ_ST_OK and results[i].dst_len == expected_size. */
#define ALZ_BRUTE_DECODERS 19
const char* alz_brute_decoder_name(uint32_t i);   /* the names of GetRawDecodersList (:96-131), e.g. "LZSS (10, 6, 2)" */
int alz_brute_force(alz_ctx* ctx, const uint8_t* raw, size_t raw_len, uint32_t expected_size,
                    uint8_t* dst, size_t slot, alz_result* results /* [ALZ_BRUTE_DECODERS] */);

#ifdef __cplusplus
}
#endif
#endif /* AURORALZ_H */
