// alz_measure.hip -- gfx950 measure kernels: a stream's alz_result WITHOUT its bytes.
//
// A measure kernel walks a stream's tokens exactly as the decoder does -- the parsers of alz_decode_serial.h and the
// lane-parallel parse rounds of alz_decode_fast.h, included as they are -- on a COUNTING sink: no OutWin, no LDS window, no
// byte phase, no store to HBM except the 16 bytes of the result.  What a token does to the output position (E5: clip_token
// against dst_cap) and to the parser state is all that is kept, so status, dst_len and src_used come out as
// alz_decode_batch reports them for the same alz_stream, for every dst_cap.  dst_off is never read.
//
// Grid mapping: one wavefront per stream, ALZ_MEASURE_WPB wavefronts (= streams) per workgroup.  The wavefronts of a workgroup
// never interact; they share a workgroup because a wavefront here needs ~1.3 KB of LDS (token staging + two 512-byte input
// chunks) and few registers, and a CU holds more of them than it holds single-wave workgroups.  The parse of one stream is a
// chain of dependent scalar steps: resident wavefronts are what buys throughput.
#include <hip/hip_runtime.h>

#include "alz_decode_fast.h"
#include "alz_measure.h"

#ifndef ALZ_MEASURE_WPB
#define ALZ_MEASURE_WPB 4
#endif

// ------------------------------------------------------------------------------------------------
// The counting sink: the sink interface of alz_decode_serial.h (DirectSink / QueueSink) with the byte work left out.
// CountOut stands where the parsers' clip_token expects an output window: the bytes "produced" so far and the capacity.
struct CountOut { u32 produced, cap; };
struct CountSink {
    CountOut& out; DecState& s;
    __device__ __forceinline__ CountSink(CountOut& o, DecState& st) : out(o), s(st) {}
    __device__ __forceinline__ u32 produced() const { return out.produced; }
    __device__ __forceinline__ void ensure(InCache& in, u32 p, u32 need) { in.ensure(p, need); }
    __device__ __forceinline__ bool lit(u32) { if (clip_token(out, s, 1) < 1) return false; out.produced += 1u; return true; }
    __device__ __forceinline__ bool match(u32, u64 len, u32) { out.produced += clip_token(out, s, len); return !s.ovf; }
    __device__ __forceinline__ bool run(InCache&, u32, u64 len) { out.produced += clip_token(out, s, len); return !s.ovf; }   // (the literals are never looked at)
    __device__ __forceinline__ void flush() {}
};

__device__ __forceinline__ void measure_write(alz_result* r, int lane, u32 produced, u32 src_used, int status, u32 src_len) {
    if (status == ALZ_ST_INPUT_TRUNCATED) src_used = src_len;         // (as write_result of the decode kernels: include/auroralz.h fixes it)
    if (lane == 0) { r->dst_len = produced; r->src_used = src_used; r->status = status; r->reserved = 0; }
}

// ------------------------------------------------------------------------------------------------
// All 25 formats, exact: the body of alz_decode_serial_kernel on the counting sink.  LDS = the input caches only (512-byte
// chunks; 256-byte ones for the formats with two or three cursors).
template <int FMT>
__global__ __launch_bounds__(64 * ALZ_MEASURE_WPB) void alz_measure_exact_kernel(const u8* __restrict__ src_base, const alz_stream* __restrict__ streams,
                                                                                 const u32* __restrict__ index_list, u32 count,
                                                                                 alz_result* __restrict__ results, alz_lz_properties lz) {
    constexpr bool TWO = (FMT == ALZ_FMT_SMSR00), THREE = (FMT == ALZ_FMT_YAY0 || FMT == ALZ_FMT_MIO0);
    constexpr int NC = THREE ? 3 : (TWO ? 2 : 1);
    constexpr u32 CH = NC > 1 ? 256u : 512u, CACHE = 2u * CH + 32u;
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_MEASURE_WPB][NC * CACHE];
    const u32 wid = (u32)threadIdx.x >> 6;
    const u32 bid = blockIdx.x * ALZ_MEASURE_WPB + wid;
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    const u32 src_len = uni(st.src_len), size = uni(st.decom_len), cap = uni(st.dst_cap);
    u8* inc_lds = lds_all[wid];
    InCache in; in.init(src, src_len, inc_lds, lane, CH);
    DecState s; dec_state_init(s);
    CountOut out; out.produced = 0; out.cap = cap;
    typedef CountSink SK;
    SK sk(out, s);
    bool has_size = false; u32 used = 0; bool used_set = false;

    if constexpr (FMT == ALZ_FMT_LZSS) {
        has_size = true;
        dec_lzss_serial(in, sk, s, src_len, size, lz.length_bits, lz.min_length, lz.windows_start, lz.max_distance, 1u << lz.window_bits);
    } else if constexpr (FMT == ALZ_FMT_LZ10) {
        has_size = true; dec_lz1x_serial<SK, false>(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_LZ11) {
        has_size = true; dec_lz1x_serial<SK, true>(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_CLZ0) {
        has_size = true; dec_clz0_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_LZ40) {
        has_size = true; dec_lz40_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_LZHUDSON) {
        has_size = true; dec_lzhudson_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_SMSR00) {
        has_size = true;
        const u32 a0 = uni(st.aux0);
        if (a0 > src_len) s.eof = true;                                   // ReadExactly(buffer, 0, codesLength) throws  SMSR00.cs:76
        else {
            InCache uin;
            uin.init(src, src_len, inc_lds + CACHE, lane, CH); uin.seek(a0 < src_len ? a0 : 0);
            dec_smsr00_serial(in, uin, sk, s, src_len, size, a0, used);
            used_set = true;
        }
    } else if constexpr (FMT == ALZ_FMT_YAZ0) {
        has_size = true; dec_yaz0_serial(in, sk, s, src_len, size);
    } else if constexpr (THREE) {
        has_size = true;
        const u32 a0 = uni(st.aux0), a1 = uni(st.aux1);
        if (FMT == ALZ_FMT_YAY0 && (a0 > src_len || a1 > src_len)) s.eof = true;   // Slice() throws  Yay0.cs:102-103
        else {
            InCache cin, uin;
            cin.init(src, src_len, inc_lds + CACHE, lane, CH); cin.seek(a0 < src_len ? a0 : 0);
            uin.init(src, src_len, inc_lds + 2 * CACHE, lane, CH); uin.seek(a1 < src_len ? a1 : 0);
            used = dec_3cursor_serial<SK, FMT == ALZ_FMT_MIO0>(in, cin, uin, sk, s, src_len, size, 0, a0, a1);
            used_set = true;
        }
    } else if constexpr (FMT == ALZ_FMT_PRS_BE) {
        dec_prs_serial<SK, true>(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_PRS_LE) {
        dec_prs_serial<SK, false>(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_LZ4_BLOCK) {
        // (history, alz_stream.aux0: bytes in front of the stream read as zeros at worst, never as an error -- E2 --, so a block with
        // history counts like one without; dst_len is the block's own bytes either way)
        dec_lz4_serial(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_LZO) {
        LzoState ls; lzo_state_init(ls);
        dec_lzo_serial(in, sk, s, src_len, ls);
    } else if constexpr (FMT == ALZ_FMT_SNAPPY_RAW) {
        u32 sz = 0; bool have = false;
        dec_snappy_serial(in, sk, s, src_len, sz, have);
    } else if constexpr (FMT == ALZ_FMT_FASTLZ) {
        FastlzState fz; fastlz_state_init(fz);
        dec_fastlz_serial(in, sk, s, src_len, fz);
    } else if constexpr (FMT == ALZ_FMT_CNX2) {
        has_size = true; dec_cnx2_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_HIG) {
        has_size = true; dec_hig_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_LZSHREK) {
        has_size = true; dec_lzshrek_serial(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_WFLZ || FMT == ALZ_FMT_WFLZ_BE) {
        dec_wflz_serial<SK, FMT == ALZ_FMT_WFLZ_BE>(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_REFPACK) {
        has_size = true; dec_refpack_serial(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_LZ02) {
        has_size = true; dec_lz02_serial(in, sk, s, src_len);
    } else if constexpr (FMT == ALZ_FMT_CNS) {
        has_size = true; dec_cns_serial(in, sk, s, src_len, size);
    } else if constexpr (FMT == ALZ_FMT_BLZ) {
        has_size = true; dec_blz_serial(in, sk, s, src_len, size < cap ? size : cap);
    }
    int status = resolve_status(s, has_size, out.produced, size, cap);
    if (FMT == ALZ_FMT_BLZ && status == ALZ_ST_OK && out.produced != size) status = ALZ_ST_OUTPUT_SIZE_MISMATCH;   // the span must be full  BLZ.cs:131
    measure_write(&results[sid], lane, out.produced, used_set ? used : s.p, status, src_len);
}

// ------------------------------------------------------------------------------------------------
// Lane-parallel bulk for the bodies without a size field (PRS, LZ4 block, LZO, raw Snappy, FastLZ, WFLZ): the loop of
// alz_decode_queue_kernel with the byte phase removed.  While a cache chunk + 76 input bytes remain a *_parse_round yields the
// bytes its tokens produce (`total`) and the input they cover (`adv`); the round is taken while its output stays within the
// capacity (Snappy: and the declared size) -- those rules, every token a round declines and the stream's tail belong to the
// exact parser on the counting sink, one token at a time (the whole tail at once), exactly as in the decoder.
// LDS per wavefront: 256 B of token staging + the input cache (two 512-byte chunks).  The parse rounds index the cache with
// (offset & 2047) for lanes whose speculation is discarded: ALZ_MEASURE_PAD keeps those reads inside the workgroup's allocation.
#define ALZ_MEASURE_PAD 1024u
template <int FMT>
__global__ __launch_bounds__(64 * ALZ_MEASURE_WPB) void alz_measure_bulk_kernel(const u8* __restrict__ src_base, const alz_stream* __restrict__ streams,
                                                                                const u32* __restrict__ index_list, u32 count,
                                                                                alz_result* __restrict__ results) {
    constexpr bool PRS = (FMT == ALZ_FMT_PRS_BE || FMT == ALZ_FMT_PRS_LE);
    constexpr u32 QCH = 512u, QCACHE = 2u * QCH + 32u, QAHEAD = QCH + 76u, PER = 256u + QCACHE;
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_MEASURE_WPB * PER + ALZ_MEASURE_PAD];
    const u32 wid = (u32)threadIdx.x >> 6;
    const u32 bid = blockIdx.x * ALZ_MEASURE_WPB + wid;
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    u8* const lds = lds_all + wid * PER;
    u32* stage = reinterpret_cast<u32*>(lds);
    InCache in; in.init(src, src_len, lds + 256, lane, QCH);
    DecState s; dec_state_init(s);
    CountOut out; out.produced = 0; out.cap = cap;
    typedef CountSink SK;
    SK sk(out, s);
    u32 qt, nt, total, adv;                                       // a round's tokens are not kept: only what they add up to
    (void)stage;
    if constexpr (PRS) {
        constexpr bool BIG = (FMT == ALZ_FMT_PRS_BE);
        u32 fl = 1u;                                              // normalised flag register (no bits pending)
        for (;;) {
            if (s.p + QAHEAD <= src_len && !s.done) {
                in.ensure(s.p, QCH);
                u32 fl2, term;
                if (prs_parse_round<BIG>(in, s.p, fl, stage, lane, qt, nt, total, adv, fl2, term) && total <= cap - out.produced) {   // the capacity rule (E5) stays with the exact parser
                    out.produced += total; s.p += adv; fl = fl2;
                    if (term) { s.done = true; break; }           // PRS.cs:78-79: the zero word ends the stream
                    continue;
                }
            }
            const bool tail = s.p + QAHEAD > src_len;
            prs_from_norm<BIG>(fl, s.bits, s.flag);
            dec_prs_serial<SK, BIG>(in, sk, s, src_len, tail ? 0xFFFFFFFFu : 1u);
            fl = prs_to_norm<BIG>(s.bits, s.flag);
            if (tail || s.eof || s.ovf || s.bad || s.done) break;
        }
    } else if constexpr (FMT == ALZ_FMT_LZ4_BLOCK) {
        for (;;) {
            if (s.p + QAHEAD <= src_len) {
                in.ensure(s.p, QCH);
                if (lz4_parse_round(in, s.p, stage, lane, qt, nt, total, adv) && total <= cap - out.produced) { out.produced += total; s.p += adv; continue; }
            }
            const bool tail = s.p + QAHEAD > src_len;
            dec_lz4_serial(in, sk, s, src_len, tail ? 0xFFFFFFFFu : 1u);
            if (tail || s.eof || s.ovf || s.bad || s.done) break;
        }
    } else if constexpr (FMT == ALZ_FMT_LZO) {
        LzoState ls; lzo_state_init(ls);
        for (;;) {
            if (ls.started && s.p + QAHEAD <= src_len) {
                in.ensure(s.p, QCH);
                u32 state = ls.plain == 0u ? 0u : (ls.plain <= 3u ? 1u : 2u);      // the walk's state in front of the round (LzoRounds)
                if (lzo_parse_round(in, s.p, stage, lane, state, qt, nt, total, adv) && total <= cap - out.produced) {
                    out.produced += total; s.p += adv;
                    ls.plain = state == 0u ? 0u : (state == 1u ? 1u : 4u);         // commit(): the state behind it
                    continue;
                }
            }
            const bool tail = s.p + QAHEAD > src_len;
            dec_lzo_serial(in, sk, s, src_len, ls, tail ? 0xFFFFFFFFu : 1u);
            if (tail || s.eof || s.ovf || s.bad || s.done) break;
        }
    } else if constexpr (FMT == ALZ_FMT_FASTLZ) {
        FastlzState fz; fastlz_state_init(fz);
        for (;;) {
            if (fz.started && s.p + QAHEAD <= src_len) {
                in.ensure(s.p, QCH);
                if (fastlz_parse_round(in, s.p, lane, fz.level, qt, nt, total, adv) && total <= cap - out.produced) { out.produced += total; s.p += adv; continue; }
            }
            const bool tail = s.p + QAHEAD > src_len;
            dec_fastlz_serial(in, sk, s, src_len, fz, tail ? 0xFFFFFFFFu : 1u);
            if (tail || s.eof || s.ovf || s.bad || s.done) break;
        }
    } else if constexpr (FMT == ALZ_FMT_WFLZ || FMT == ALZ_FMT_WFLZ_BE) {
        constexpr bool BIG = (FMT == ALZ_FMT_WFLZ_BE);
        for (;;) {
            if (s.p + QAHEAD <= src_len) {
                in.ensure(s.p, QCH);
                if (out.produced < cap && wflz_parse_round<BIG>(in, s.p, stage, lane, qt, nt, total, adv) && total <= cap - out.produced) { out.produced += total; s.p += adv; continue; }
            }
            const bool tail = s.p + QAHEAD > src_len;
            dec_wflz_serial<SK, BIG>(in, sk, s, src_len, tail ? 0xFFFFFFFFu : 1u);
            if (tail || s.eof || s.ovf || s.bad || s.done) break;
        }
    } else {
        // Snappy: varint size, then elements until the output reaches it
        u32 size = 0; bool have = false;
        for (;;) {
            if (have && s.p + QAHEAD <= src_len) {
                in.ensure(s.p, QCH);
                if (out.produced >= size) break;
                const u32 maxout = size < cap ? size : cap;
                if (out.produced < cap && snappy_parse_round(in, s.p, lane, qt, nt, total, adv) && total <= maxout - out.produced) { out.produced += total; s.p += adv; continue; }
            }
            const bool tail = s.p + QAHEAD > src_len;
            dec_snappy_serial(in, sk, s, src_len, size, have, tail ? 0xFFFFFFFFu : 1u);
            if (tail || s.eof || s.ovf || s.bad || out.produced >= size) break;
        }
    }
    measure_write(&results[sid], lane, out.produced, s.p, resolve_status(s, false, out.produced, 0u, cap), src_len);
}

// ------------------------------------------------------------------------------------------------
template <int FMT>
static hipError_t launch_exact(hipStream_t stream, const u8* s, const alz_stream* streams, const u32* index, u32 count, alz_result* results, const alz_lz_properties& lz) {
    hipLaunchKernelGGL((alz_measure_exact_kernel<FMT>), dim3((count + ALZ_MEASURE_WPB - 1) / ALZ_MEASURE_WPB), dim3(64 * ALZ_MEASURE_WPB), 0, stream, s, streams, index, count, results, lz);
    return hipGetLastError();
}
template <int FMT>
static hipError_t launch_bulk(hipStream_t stream, const u8* s, const alz_stream* streams, const u32* index, u32 count, alz_result* results) {
    hipLaunchKernelGGL((alz_measure_bulk_kernel<FMT>), dim3((count + ALZ_MEASURE_WPB - 1) / ALZ_MEASURE_WPB), dim3(64 * ALZ_MEASURE_WPB), 0, stream, s, streams, index, count, results);
    return hipGetLastError();
}

bool alz_measure_has_bulk(int fmt) {
    switch (fmt) {
    case ALZ_FMT_PRS_BE: case ALZ_FMT_PRS_LE: case ALZ_FMT_LZ4_BLOCK: case ALZ_FMT_LZO: case ALZ_FMT_SNAPPY_RAW: case ALZ_FMT_FASTLZ:
    case ALZ_FMT_WFLZ: case ALZ_FMT_WFLZ_BE: return true;
    default: return false;
    }
}

hipError_t alz_launch_measure(int fmt, hipStream_t stream, const void* src, const alz_stream* streams, const u32* index, u32 count,
                              alz_result* results, const alz_lz_properties* lzp, bool exact) {
    if (count == 0) return hipSuccess;
    const u8* s = (const u8*)src;
    const alz_lz_properties lz = *lzp;
    if (!exact) {
        switch (fmt) {
        case ALZ_FMT_PRS_BE: return launch_bulk<ALZ_FMT_PRS_BE>(stream, s, streams, index, count, results);
        case ALZ_FMT_PRS_LE: return launch_bulk<ALZ_FMT_PRS_LE>(stream, s, streams, index, count, results);
        case ALZ_FMT_LZ4_BLOCK: return launch_bulk<ALZ_FMT_LZ4_BLOCK>(stream, s, streams, index, count, results);
        case ALZ_FMT_LZO: return launch_bulk<ALZ_FMT_LZO>(stream, s, streams, index, count, results);
        case ALZ_FMT_SNAPPY_RAW: return launch_bulk<ALZ_FMT_SNAPPY_RAW>(stream, s, streams, index, count, results);
        case ALZ_FMT_FASTLZ: return launch_bulk<ALZ_FMT_FASTLZ>(stream, s, streams, index, count, results);
        case ALZ_FMT_WFLZ: return launch_bulk<ALZ_FMT_WFLZ>(stream, s, streams, index, count, results);
        case ALZ_FMT_WFLZ_BE: return launch_bulk<ALZ_FMT_WFLZ_BE>(stream, s, streams, index, count, results);
        default: break;       // every other format: the exact tier (the flag-byte family states its size in the header)
        }
    }
    switch (fmt) {
#define ALZ_MEASURE_CASE(F) case F: return launch_exact<F>(stream, s, streams, index, count, results, lz);
    ALZ_MEASURE_CASE(ALZ_FMT_LZSS) ALZ_MEASURE_CASE(ALZ_FMT_LZ10) ALZ_MEASURE_CASE(ALZ_FMT_LZ11) ALZ_MEASURE_CASE(ALZ_FMT_YAZ0)
    ALZ_MEASURE_CASE(ALZ_FMT_YAY0) ALZ_MEASURE_CASE(ALZ_FMT_MIO0) ALZ_MEASURE_CASE(ALZ_FMT_PRS_BE) ALZ_MEASURE_CASE(ALZ_FMT_PRS_LE)
    ALZ_MEASURE_CASE(ALZ_FMT_LZ4_BLOCK) ALZ_MEASURE_CASE(ALZ_FMT_LZO) ALZ_MEASURE_CASE(ALZ_FMT_SNAPPY_RAW) ALZ_MEASURE_CASE(ALZ_FMT_LZ40)
    ALZ_MEASURE_CASE(ALZ_FMT_LZHUDSON) ALZ_MEASURE_CASE(ALZ_FMT_SMSR00) ALZ_MEASURE_CASE(ALZ_FMT_FASTLZ) ALZ_MEASURE_CASE(ALZ_FMT_CNX2)
    ALZ_MEASURE_CASE(ALZ_FMT_BLZ) ALZ_MEASURE_CASE(ALZ_FMT_CLZ0) ALZ_MEASURE_CASE(ALZ_FMT_CNS) ALZ_MEASURE_CASE(ALZ_FMT_LZ02)
    ALZ_MEASURE_CASE(ALZ_FMT_REFPACK) ALZ_MEASURE_CASE(ALZ_FMT_WFLZ) ALZ_MEASURE_CASE(ALZ_FMT_WFLZ_BE) ALZ_MEASURE_CASE(ALZ_FMT_LZSHREK)
    ALZ_MEASURE_CASE(ALZ_FMT_HIG)
#undef ALZ_MEASURE_CASE
    default: return hipErrorInvalidValue;
    }
}
