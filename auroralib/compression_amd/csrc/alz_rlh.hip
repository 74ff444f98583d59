// alz_rlh.hip -- gfx950 kernels of the two non-LZ members of the Nintendo GBA / DS family: RLE30 (decode + encode) and HUF20 (decode), and of
// RLE30's sibling RLHudson (Hudson Soft's byte RLE, decode + encode: the RLE30 kernels over another grammar trait, alz_rlh_hudson_*).
// A family of its own beside decode / encode / measure (tools/kernel_hash.py "rlh"): these bodies have no window, no match copy and
// no oracle body, so they share nothing with the LZ kernels but the input cache (InCache), the wave scan and the chain walk
// (lane_walk_pos) of alz_decode_fast.h, included as they are.  Citations are relative to the reference's
// src/AuroraLib.Compression.Nintendo (Nintendo/RLE30.cs, Nintendo/HUF20.cs, HudsonSoft/RLHudson.cs) and src/AuroraLib.Compression
// (MatchFinder/RleMatchFinder.cs).
//
// Grid mapping: one wavefront per stream, ALZ_RLH_WPB wavefronts (= streams) per workgroup; the wavefronts of a workgroup never
// interact.  Control flow is wave-uniform (parse state through readfirstlane), the 64 lanes share the byte work.
//
// Two families per alz_ctx_set_exact_kernels:
//   exact       one token (RLE30) / one bit (HUF20) at a time: the statement-for-statement restatement.
//   production  RLE30 / RLHudson decode: where the element that starts at input byte p ends is a function of byte p alone (p + 2 for a run,
//               p + n + 1 for n literals; RLHudson's `80`, no literals in one byte, is left to the exact step), so every lane sizes "the
//               element that would start at my byte" of a 256-byte window, the chain walk finds the real starts, output offsets are a prefix sum over the element lengths, and the round's bytes are
//               written back in aligned 16-byte granules, one per lane (a run is a broadcast of one byte, a literal run a copy out of
//               the input cache).  The stream's tail, the token that meets dst_cap and every error end in the exact step.
//               HUF20 decode: lanes decode consecutive 32-bit words speculatively from the root state, then re-decode from their
//               left neighbour's exit state until nothing changes (bounded; fixed-length codes never self-synchronise and take
//               the full bound), symbols per lane are prefix-summed and written per output byte.  A round that does not settle, the
//               tail and every error go to the exact path.
//               RLE30 / RLHudson encode: one kernel for both families (run lengths and the literal walk of TryToFindMatch by ballots over
//               128 positions, one token per step).
#include <hip/hip_runtime.h>

#include "alz_decode_fast.h"
#include "alz_rlh.h"

#ifndef ALZ_RLH_WPB
#define ALZ_RLH_WPB 4
#endif

__device__ __forceinline__ void rlh_write(alz_result* r, int lane, u32 dst_len, u32 src_used, int status) {
    if (lane == 0) { r->dst_len = dst_len; r->src_used = src_used; r->status = status; r->reserved = 0; }
}

// ------------------------------------------------------------------------------------------------ RLE30 / RLHudson decode
// The two byte RLEs differ in their grammar only, which a trait carries: which half of the control bytes is a run (polarity), the length bias,
// and whether an element may produce nothing.  Everything else -- the token step, the finish, the lane-parallel round -- is written once.
//   RLE30     c >= 0x80: the next byte (c & 0x7F) + 3 times, else (c & 0x7F) + 1 literals; end of input reads as a literal run  RLE30.cs:84-98
//   RLHudson  c <  0x80: the next byte (c & 0x7F) times, else (c & 0x7F) literals, both may be 0; ReadByte() = -1 reads as a run of 127
//             whose ReadUInt8 throws  HudsonSoft/RLHudson.cs:60-75
struct Rle30Grammar {
    static constexpr bool kZeroLen = false;                              // every element writes at least one byte
    __device__ static __forceinline__ bool run(u32 c) { return c >= 0x80u; }                          // :87
    __device__ static __forceinline__ u32 len(u32 c) { return (c & 0x7Fu) + (c >= 0x80u ? 3u : 1u); } // :85, :90
    // input bytes of the element that starts with control byte b, for the chain walk
    __device__ static __forceinline__ u32 size(u32 b) { return b >= 0x80u ? 2u : b + 2u; }            // control + byte | control + (b + 1) literals
    // the encoder's control bytes  RLE30.cs:119, :124 (a literal run of 129 -> 0x80: the defect)
    __device__ static __forceinline__ u8 ctl_run(u32 dur) { return (u8)((dur - 3u) | 0x80u); }
    __device__ static __forceinline__ u8 ctl_lit(u32 dur) { return (u8)(dur - 1u); }
};
struct HudsonGrammar {
    static constexpr bool kZeroLen = true;                               // `00 xx` is two bytes that write nothing
    __device__ static __forceinline__ bool run(u32 c) { return c < 0x80u; }                           // RLHudson.cs:65
    __device__ static __forceinline__ u32 len(u32 c) { return c & 0x7Fu; }                            // :63
    // `80`, no literals, is the one element of a single byte: the walk's bound of 32 elements per 64-byte sub-window needs two, so it is an
    // unusual element and the exact step's
    __device__ static __forceinline__ u32 size(u32 b) { return b < 0x80u ? 2u : (b == 0x80u ? ALZ_NX_BAD : (b & 0x7Fu) + 1u); }
    // the encoder's control bytes  RLHudson.cs:92, :97 (literal runs of 128 / 129 -> 0x80 / 0x81: the defect)
    __device__ static __forceinline__ u8 ctl_run(u32 dur) { return (u8)dur; }
    __device__ static __forceinline__ u8 ctl_lit(u32 dur) { return (u8)(dur | 0x80u); }
};

struct RleState { u32 p, o; bool eof, ovf; u64 attempted_end; };

// DecompressHeaderless, one pass of its loop (RLE30.cs:84-98, RLHudson.cs:62-74), read from global memory.  false: decoding ends here.
template <class G>
__device__ __forceinline__ bool rle_token(const u8* __restrict__ src, u32 n, u8* __restrict__ dst, u32 cap, int lane, RleState& s) {
    if (s.p >= n) { s.eof = true; return false; }                        // ReadByte() = -1: an element that cannot be read  RLE30.cs:84-96, RLHudson.cs:62-67
    const u32 c = uni((u32)src[s.p]);
    const u32 len = G::len(c);
    const bool run = G::run(c);
    const u32 left = n - s.p - 1u;                                       // input behind the control byte
    if (run) { if (left < 1u) { s.eof = true; return false; } }          // ReadUInt8 throws, also in front of a run of 0  RLE30.cs:90, RLHudson.cs:67
    else if (left < len) { s.eof = true; return false; }                 // Read(section) != length (nothing of the short run is written)  RLE30.cs:95-96, RLHudson.cs:71-72
    const u32 room = cap - s.o, cl = len < room ? len : room;            // E5
    if (run) {
        const u32 b = uni((u32)src[s.p + 1u]);
        for (u32 k = (u32)lane; k < cl; k += 64u) dst[s.o + k] = (u8)b;  // section.Fill
        s.p += 2u;
    } else {
        for (u32 k = (u32)lane; k < cl; k += 64u) dst[s.o + k] = src[s.p + 1u + k];
        s.p += 1u + len;
    }
    if (len > room) { s.ovf = true; s.attempted_end = (u64)s.o + len; s.o = cap; return false; }
    s.o += len;                                                          // RLE30.cs:98, RLHudson.cs:74
    return true;
}

__device__ __forceinline__ void rle_finish(alz_result* r, int lane, const RleState& s, u32 n, u32 size, u32 cap) {
    int status = ALZ_ST_OK;
    if (s.eof) status = ALZ_ST_INPUT_TRUNCATED;
    else if (s.ovf) status = (s.attempted_end > (u64)size && cap >= size) ? ALZ_ST_OUTPUT_SIZE_MISMATCH : ALZ_ST_OUTPUT_CAPACITY;
    else if (s.o > size) status = ALZ_ST_OUTPUT_SIZE_MISMATCH;           // RLE30.cs:101-104, RLHudson.cs:77-80
    rlh_write(r, lane, s.o, s.eof ? n : s.p, status);
}

// the exact family: one token per step
template <class G>
__device__ __forceinline__ void rle_decode_exact(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                 const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results) {
    const u32 bid = blockIdx.x * ALZ_RLH_WPB + ((u32)threadIdx.x >> 6);
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    u8* dst = dst_base + st.dst_off;
    const u32 n = uni(st.src_len), size = uni(st.decom_len), cap = uni(st.dst_cap);
    RleState s; s.p = 0; s.o = 0; s.eof = false; s.ovf = false; s.attempted_end = 0;
    while (s.o < size)                                                   // RLE30.cs:82, RLHudson.cs:60
        if (!rle_token<G>(src, n, dst, cap, lane, s)) break;
    rle_finish(&results[sid], lane, s, n, size, cap);
}

// LDS per wavefront: the input cache (two 512-byte chunks + 32) and the round's element table (64 ends + 64 descriptors).
#define ALZ_RLH_QCH 512u
#define ALZ_RLH_CACHE (2u * ALZ_RLH_QCH + 32u)
#define ALZ_RLH_RLE_PER (ALZ_RLH_CACHE + 512u)
// the production family; lds_all: ALZ_RLH_WPB * ALZ_RLH_RLE_PER bytes of the workgroup
template <class G>
__device__ __forceinline__ void rle_decode_rounds(u8* lds_all, const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                  const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results) {
    const u32 wid = (u32)threadIdx.x >> 6;
    const u32 bid = blockIdx.x * ALZ_RLH_WPB + wid;
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    u8* dst = dst_base + st.dst_off;
    const u32 n = uni(st.src_len), size = uni(st.decom_len), cap = uni(st.dst_cap);
    u8* const lds = lds_all + wid * ALZ_RLH_RLE_PER;
    u32* const tend = reinterpret_cast<u32*>(lds + ALZ_RLH_CACHE);       // inclusive output end of element j, relative to the round
    u32* const tdesc = tend + 64;                                        // bit 31: a run of (bits 0..7); else the input-cache index of its first literal
    InCache in; in.init(src, n, lds, lane, ALZ_RLH_QCH);
    RleState s; s.p = 0; s.o = 0; s.eof = false; s.ovf = false; s.attempted_end = 0;
    while (s.o < size) {
        // a round needs its 256-byte window and the longest element that can start in it (1 + 128 bytes) inside the input: the tail is the exact step's
        if ((u64)s.p + ALZ_RLH_QCH + 76u <= (u64)n) {
            in.ensure(s.p, ALZ_RLH_QCH);
            const u32 i0 = in.idx(s.p);
            u32 nx[4];
#pragma unroll
            for (int w = 0; w < 4; w++) nx[w] = G::size((u32)in.lds[i0 + 64u * (u32)w + (u32)lane]);
            u32 spos, sp, nel;
            // lane_walk_pos walks four 64-byte sub-windows and records element j's start in lane j (v_writelane, lane index in m0).  A sub-window is
            // entered only while fewer than 33 elements are taken, and adds at most 32 (every element it takes has >= 2 bytes): at most 32 + 32 = 64
            // elements, so the lane index stays <= 63 and never wraps to lane 0.
            lane_walk_pos(nx, 33u, spos, sp, nel);
            const u32 pos = i0 + (spos & 255u);
            const u32 b = in.lds[pos], e1 = in.lds[pos + 1u];
            const bool mine = (u32)lane < nel;
            const u32 len = !mine ? 0u : G::len(b);
            const u32 incl = wave_incl_scan(len, lane), excl = incl - len;
            // elements are taken while the output is short of the declared size (the loop condition) and they fit dst_cap whole (E5 is the exact step's)
            const u64 takem = wave_ballot(mine && excl < size - s.o && incl <= cap - s.o);
            const u32 k = (u32)__popcll(takem);
            if (k) {
                const u32 total = wave_readlane(incl, k - 1u);
                const u32 adv = k == nel ? sp : (wave_readlane(spos, k) & 255u);
                tend[lane] = incl; tdesc[lane] = G::run(b) ? (0x80000000u | e1) : pos + 1u;
                wave_sync();
                u8* const o = dst + s.o;
                const u32 a0 = (u32)(reinterpret_cast<uintptr_t>(o) & 15u);
                const u32 ng = (G::kZeroLen && total == 0u) ? 0u : (a0 + total + 15u) >> 4;   // (a round of empty runs only moves the input on)
                for (u32 g = (u32)lane; g < ng; g += 64u) {              // one aligned 16-byte granule per lane and pass
                    const int k0 = (int)(g << 4) - (int)a0;
                    const u32 kb = k0 < 0 ? 0u : (u32)k0, ke = (u32)(k0 + 16) < total ? (u32)(k0 + 16) : total;
                    u32 lo = 0u, hi = k - 1u;                            // the element of byte kb: the first whose end lies behind it
#pragma unroll
                    for (int it = 0; it < 6; it++) {
                        const u32 mid = (lo + hi) >> 1;
                        if (lo < hi) { if (tend[mid] > kb) hi = mid; else lo = mid + 1u; }
                    }
                    u32 t = lo, te = tend[t], ts = t ? tend[t - 1u] : 0u, d = tdesc[t];
                    u32 w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        const u32 q = (u32)(k0 + j);
                        if (k0 + j >= (int)kb && q < ke) {
                            if (G::kZeroLen) { while (q >= te) { ts = te; t++; te = tend[t]; d = tdesc[t]; } }   // q < total = tend[k - 1]: stops inside the table
                            else if (q >= te) { ts = te; t++; te = tend[t]; d = tdesc[t]; }                     // (every element has at least one byte)
                            const u32 v = (d >> 31) ? (d & 0xFFu) : (u32)in.lds[d + (q - ts)];
                            w[j >> 2] |= v << (8 * (j & 3));
                        }
                    }
                    if (k0 >= 0 && (u32)(k0 + 16) <= total) *reinterpret_cast<uint4*>(o + k0) = make_uint4(w[0], w[1], w[2], w[3]);
                    else {
#pragma unroll
                        for (int j = 0; j < 16; j++)
                            if (k0 + j >= (int)kb && (u32)(k0 + j) < ke) o[k0 + j] = (u8)(w[j >> 2] >> (8 * (j & 3)));
                    }
                }
                wave_sync();
                s.o += total; s.p += adv;
                continue;
            }
        }
        if (!rle_token<G>(src, n, dst, cap, lane, s)) break;
    }
    rle_finish(&results[sid], lane, s, n, size, cap);
}

#define ALZ_RLH_KERNEL_ARGS const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams, \
                            const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_rle30_decode_exact_kernel(ALZ_RLH_KERNEL_ARGS) {
    rle_decode_exact<Rle30Grammar>(src_base, dst_base, streams, index_list, count, results);
}
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_hudson_decode_exact_kernel(ALZ_RLH_KERNEL_ARGS) {
    rle_decode_exact<HudsonGrammar>(src_base, dst_base, streams, index_list, count, results);
}
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_rle30_decode_kernel(ALZ_RLH_KERNEL_ARGS) {
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_RLH_WPB * ALZ_RLH_RLE_PER];
    rle_decode_rounds<Rle30Grammar>(lds_all, src_base, dst_base, streams, index_list, count, results);
}
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_hudson_decode_kernel(ALZ_RLH_KERNEL_ARGS) {
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_RLH_WPB * ALZ_RLH_RLE_PER];
    rle_decode_rounds<HudsonGrammar>(lds_all, src_base, dst_base, streams, index_list, count, results);
}

// ------------------------------------------------------------------------------------------------ RLE30 / RLHudson encode
// RLE30.CompressHeaderless (RLE30.cs:110-129) and RLHudson.CompressHeaderless (RLHudson.cs:83-102), both over RleMatchFinder(3, 127).TryToFindMatch
// (RleMatchFinder.cs:29-51), one token per step: the 127 candidate positions of a step are two ballots of 64.  The two differ in the control bytes
// only (the grammar trait).  The managed defect is kept: `duration = source.Length - offset` (:43) makes a literal run of up to 129 bytes, whose
// control byte wraps -- RLE30's (duration - 1) to 0x80, RLHudson's (duration | 0x80) to 0x80 / 0x81 for 128 / 129.
// Over dst_cap: status OUTPUT_CAPACITY and dst_len 0, as the LZ encoders report it; nothing behind dst_cap is written.
template <class G>
__device__ __forceinline__ void rle_encode(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                           const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results) {
    const u32 bid = blockIdx.x * ALZ_RLH_WPB + ((u32)threadIdx.x >> 6);
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    u8* dst = dst_base + st.dst_off;
    const u32 n = uni(st.src_len), cap = uni(st.dst_cap);
    u32 p = 0, q = 0; bool fail = false;
    while (p < n) {                                                      // RLE30.cs:115, RLHudson.cs:88
        const u32 rem = n - p;
        const u32 b0 = uni((u32)src[p]);
        const u32 lim = rem < 127u ? rem : 127u;                         // RleMatchFinder.cs:31
        // GetRelMatchLength (:53-64): the first i in 1..lim-1 whose byte differs, else lim
        u32 dur;
        {
            const u32 i1 = 1u + (u32)lane;
            const u64 m1 = wave_ballot(i1 >= lim || src[p + i1] != b0);
            if (m1) dur = 1u + (u32)__builtin_ctzll(m1);
            else {
                const u32 i2 = 65u + (u32)lane;
                const u64 m2 = wave_ballot(i2 >= lim || src[p + i2] != b0);   // (lim <= 127: lane 62 always stops)
                dur = 65u + (u32)__builtin_ctzll(m2);
            }
        }
        const bool run = dur >= 3u;                                      // :34
        if (!run) {
            // the do-while of :37-47: the first d in 1..127 with  rem - d < 3 (then d = rem)  |  d == 127  |  three equal bytes at p + d
            u32 d;
            {
                const u32 d1 = 1u + (u32)lane;
                bool stop = rem < d1 + 3u || d1 == 127u;
                if (!stop) { const u32 x = src[p + d1]; stop = src[p + d1 + 1u] == x && src[p + d1 + 2u] == x; }
                const u64 m1 = wave_ballot(stop);
                if (m1) d = 1u + (u32)__builtin_ctzll(m1);
                else {
                    const u32 d2 = 65u + (u32)lane;
                    bool stop2 = rem < d2 + 3u || d2 >= 127u;
                    if (!stop2) { const u32 x = src[p + d2]; stop2 = src[p + d2 + 1u] == x && src[p + d2 + 2u] == x; }
                    d = 65u + (u32)__builtin_ctzll(wave_ballot(stop2));
                }
            }
            dur = rem < d + 3u ? rem : d;                                // :41-45 comes first inside the loop body
        }
        const u32 tb = run ? 2u : 1u + dur;
        if ((u64)q + tb > (u64)cap) { fail = true; break; }
        if (run) {
            if (lane == 0) { dst[q] = G::ctl_run(dur); dst[q + 1u] = (u8)b0; }   // RLE30.cs:119-120, RLHudson.cs:92-93
        } else {
            if (lane == 0) dst[q] = G::ctl_lit(dur);                     // RLE30.cs:124, RLHudson.cs:97
            for (u32 k = (u32)lane; k < dur; k += 64u) dst[q + 1u + k] = src[p + k];   // RLE30.cs:125, RLHudson.cs:98
        }
        q += tb; p += dur;                                               // RLE30.cs:127, RLHudson.cs:100
    }
    rlh_write(&results[sid], lane, fail ? 0u : q, n, fail ? ALZ_ST_OUTPUT_CAPACITY : ALZ_ST_OK);
}
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_rle30_encode_kernel(ALZ_RLH_KERNEL_ARGS) {
    rle_encode<Rle30Grammar>(src_base, dst_base, streams, index_list, count, results);
}
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_hudson_encode_kernel(ALZ_RLH_KERNEL_ARGS) {
    rle_encode<HudsonGrammar>(src_base, dst_base, streams, index_list, count, results);
}

// ------------------------------------------------------------------------------------------------ HUF20 decode
// HUF20.DecompressHeaderless (HUF20.cs:94-152).  The tree (treeSize * 2 <= 510 bytes; a short read leaves zeros, :100-101) sits in LDS.
struct HufState {
    u32 p;          // input offset just behind the last word read
    u32 flag, bits; // current word, bits not yet consumed
    u32 pos, nxt;   // treePos, next  :117
    u32 i;          // symbols emitted
    bool eof, oob;
};

// reads the two header bytes and the tree; false: a header byte is missing (ReadUInt8 throws, :98-99)
__device__ __forceinline__ bool huf20_header(const u8* __restrict__ src, u32 n, u8* tree, int lane, u32& tlen, u32& root, u32& p) {
    if (n < 2u) return false;
    const u32 hdr = (u32)src[0] | ((u32)src[1] << 8);
    tlen = 2u * uni(hdr & 0xFFu); root = uni(hdr >> 8);
    const u32 have = n - 2u < tlen ? n - 2u : tlen;                      // source.Read(tree): short is no error  :101
#pragma unroll
    for (u32 k = 0; k < 512u; k += 64u) tree[k + (u32)lane] = (k + (u32)lane) < have ? src[2u + k + (u32)lane] : (u8)0;
    wave_sync();
    p = 2u + have;
    return true;
}

// One symbol's bits from the state `h` on, exact (:126-150); the emitted tree byte in `sym`.  false: decoding ends (h.eof / h.oob).
__device__ __forceinline__ bool huf20_symbol(InCache& in, u32 n, const u8* tree, u32 tlen, u32 root, HufState& h, u32& sym) {
    for (;;) {
        if (h.bits == 0u) {                                              // :126-130
            if ((u64)h.p + 4u > (u64)n) { h.eof = true; return false; }
            in.ensure(h.p, 4u);
            h.flag = in.peek4(h.p); h.p += 4u; h.bits = 32u;
        }
        h.nxt += ((h.pos & 0x3Fu) << 1) + 2u;                            // :132
        h.bits -= 1u;
        const u32 dir = 2u - ((h.flag >> h.bits) & 1u);                  // :133
        const u32 leaf = (h.pos >> (5u + dir)) & 1u;                     // :134
        const u32 at = h.nxt - dir;
        if (at >= tlen) { h.oob = true; return false; }                  // IndexOutOfRangeException  :136
        h.pos = uni((u32)tree[at]);
        if (leaf) { sym = h.pos; h.pos = root; h.nxt = 0u; return true; }   // :148-149
    }
}

// The output side of both families.  Symbols arrive in order; every lane keeps one output byte of the current block of 64 and the block is
// stored when it is full.  4-bit mode ORs the WHOLE tree byte, shifted by 4 or by 0, into its output byte (:145-146): a leaf value above 0xF
// pollutes the other nibble (unshifted) or loses its high bits (shifted) as the managed code does.  Only [0, lim) is ever written.
template <bool NIB>
struct HufOut {
    u8* dst; u32 lo, lim; int lane; u32 acc; bool little;      // [lo, lim): the output bytes this sink owns (lo > 0: the lane-parallel rounds wrote what lies in front)
    __device__ __forceinline__ void put(u32 i, u32 sym) {
        const u32 j = NIB ? i >> 1 : i;
        u32 v = sym;
        if (NIB) { const bool shift = ((i & 1u) == 0u) != little; v = (sym << (shift ? 4u : 0u)) & 0xFFu; }
        if ((u32)lane == (j & 63u)) acc = NIB ? (acc | v) : v;
        const bool last = NIB ? ((i & 127u) == 127u) : ((i & 63u) == 63u);
        if (last) { const u32 o = (j & ~63u) + (u32)lane; if (o >= lo && o < lim) dst[o] = (u8)acc; acc = 0u; }
    }
    __device__ __forceinline__ void finish(u32 i) {                      // the partial block behind symbol i - 1
        const u32 jn = NIB ? (i + 1u) >> 1 : i;                          // output bytes touched so far
        if (jn & 63u) { const u32 o = (jn & ~63u) + (u32)lane; if (o >= lo && o < jn && o < lim) dst[o] = (u8)acc; }
    }
};

__device__ __forceinline__ void huf20_finish(alz_result* r, int lane, const HufState& h, bool hdr_ok, u32 n, u32 size, u32 cap) {
    int status = ALZ_ST_OK; u32 used = h.p;
    if (!hdr_ok || h.eof) { status = ALZ_ST_INPUT_TRUNCATED; used = n; }
    else if (h.oob) status = ALZ_ST_INPUT_TRUNCATED;                     // (src_used: just behind the last word read)
    else if (cap < size) status = ALZ_ST_OUTPUT_CAPACITY;                // a stream error wins over it: the managed order of events
    rlh_write(r, lane, status == ALZ_ST_OK ? size : 0u, used, status);   // :103-107: nothing is handed over unless the whole decode succeeded
}

// The exact decode from the state `h` to the end of the stream: one bit at a time on the input cache (positioned here).  `carry` (4-bit mode,
// h.i odd): the symbol in front of h.i, whose output byte is not written yet.
template <bool NIB>
__device__ __forceinline__ void huf20_exact_tail(const u8* __restrict__ src, u32 n, u8* lds, const u8* tree, u32 tlen, u32 root, HufState& h, u32 symbols,
                                                 u8* dst, u32 lim, bool little, int lane, u32 carry) {
    InCache in; in.init_at(src, n, lds, lane, ALZ_RLH_QCH, h.p);
    HufOut<NIB> out; out.dst = dst; out.lim = lim; out.lane = lane; out.acc = 0u; out.little = little;
    out.lo = NIB ? h.i >> 1 : h.i;
    if (NIB && (h.i & 1u)) out.put(h.i - 1u, carry);
    while (h.i < symbols) {                                              // :124
        u32 sym;
        if (!huf20_symbol(in, n, tree, tlen, root, h, sym)) break;
        out.put(h.i, sym); h.i += 1u;
    }
    out.finish(h.i);
}

#define ALZ_RLH_HUF_PER (ALZ_RLH_CACHE + 512u)
template <bool NIB>
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_huf20_decode_exact_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                                                     const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                                                     u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_RLH_WPB * ALZ_RLH_HUF_PER];
    const u32 wid = (u32)threadIdx.x >> 6;
    const u32 bid = blockIdx.x * ALZ_RLH_WPB + wid;
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    const u32 n = uni(st.src_len), size = uni(st.decom_len), cap = uni(st.dst_cap);
    u8* const lds = lds_all + wid * ALZ_RLH_HUF_PER;
    u8* const tree = lds + ALZ_RLH_CACHE;
    HufState h; h.p = 0; h.flag = 0; h.bits = 0; h.pos = 0; h.nxt = 0; h.i = 0; h.eof = false; h.oob = false;
    u32 tlen = 0, root = 0;
    const bool hdr_ok = huf20_header(src, n, tree, lane, tlen, root, h.p);
    if (hdr_ok) {
        h.pos = root;
        const u32 symbols = NIB ? size * 2u : size;                      // decomLength * 8 / bitDepth  :117 (decom_len < 2^28: the host refuses more)
        huf20_exact_tail<NIB>(src, n, lds, tree, tlen, root, h, symbols, dst_base + st.dst_off, cap < size ? cap : size, NIB ? uni(st.aux0) == 0u : true, lane, 0u);
    }
    huf20_finish(&results[sid], lane, h, hdr_ok, n, size, cap);
}

// ---- the lane-parallel rounds.  A round is 64 words, one per lane.  What a lane's 32 bits decode to depends on the state (treePos, next) it
// is entered with; lane 0's is known, every other lane starts from the root state (a code boundary) and then takes over its left neighbour's
// exit state until no lane changes.  Lane k is right after k sweeps at the latest, so ALZ_RLH_HUF_SWEEPS = 64 + 2 always settles; the bound is
// checked all the same.  A Huffman code re-synchronises within a few symbols, so real streams settle in two or three sweeps; fixed-length
// codes never do (3-bit codes: the entry state of a word depends on its index mod 3) and take the whole bound -- each lane keeps the last
// three (entry -> exit, count) results, so that those sweeps are a compare each and not a decode each.
// state word: treePos | next << 8.
#define ALZ_RLH_HUF_SWEEPS 66u
#define ALZ_RLH_HUF_STAGE 2080u                       /* one byte per symbol of a round (<= 64 x 32 one-bit codes) + the carried one + slack */
#define ALZ_RLH_HUFP_PER (ALZ_RLH_CACHE + 512u + ALZ_RLH_HUF_STAGE)
template <bool EMIT>
__device__ __forceinline__ void huf20_word(u32 w, u32 entry, const u8* tree, u32 tlen, u32 root, u32& exit_state, u32& cnt, bool& oob, u8* stage_at) {
    u32 pos = entry & 0xFFu, nxt = entry >> 8, c = 0u;
    bool bad = false;
    for (int b = 31; b >= 0; b--) {
        nxt += ((pos & 0x3Fu) << 1) + 2u;                                // :132
        const u32 dir = 2u - ((w >> b) & 1u);                            // :133
        const u32 leaf = (pos >> (5u + dir)) & 1u;                       // :134
        const u32 at = nxt - dir;
        if (at >= tlen) { bad = true; break; }                           // :136 out of range: the exact path reports it
        pos = tree[at];
        if (leaf) { if (EMIT) stage_at[c] = (u8)pos; c++; pos = root; nxt = 0u; }
    }
    exit_state = pos | (nxt << 8); cnt = c; oob = bad;
}

template <bool NIB>
__global__ __launch_bounds__(64 * ALZ_RLH_WPB) void alz_rlh_huf20_decode_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                                               const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                                               u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds_all[ALZ_RLH_WPB * ALZ_RLH_HUFP_PER];
    const u32 wid = (u32)threadIdx.x >> 6;
    const u32 bid = blockIdx.x * ALZ_RLH_WPB + wid;
    if (bid >= count) return;
    const int lane = (int)(threadIdx.x & 63u);
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u8* src = src_base + st.src_off;
    u8* const dst = dst_base + st.dst_off;
    const u32 n = uni(st.src_len), size = uni(st.decom_len), cap = uni(st.dst_cap);
    u8* const lds = lds_all + wid * ALZ_RLH_HUFP_PER;
    u8* const tree = lds + ALZ_RLH_CACHE;
    u8* const stage = tree + 512u;
    HufState h; h.p = 0; h.flag = 0; h.bits = 0; h.pos = 0; h.nxt = 0; h.i = 0; h.eof = false; h.oob = false;
    u32 tlen = 0, root = 0;
    const bool hdr_ok = huf20_header(src, n, tree, lane, tlen, root, h.p);
    if (hdr_ok) {
        h.pos = root;
        const u32 symbols = NIB ? size * 2u : size;
        const u32 lim = cap < size ? cap : size;
        const bool little = NIB ? uni(st.aux0) == 0u : true;
        u32 carry_n = 0u;                                                // 4-bit mode: 1 = stage[0] holds the symbol in front of h.i (h.i odd)
        while (h.i < symbols && (u64)h.p + 256u <= (u64)n) {
            u32 w;
            __builtin_memcpy(&w, src + h.p + 4u * (u32)lane, 4);         // ReadInt32: little-endian  :128
            const u32 real = h.pos | (h.nxt << 8);
            u32 entry = lane == 0 ? real : root;
            u32 ex, cn; bool ob;
            huf20_word<false>(w, entry, tree, tlen, root, ex, cn, ob, nullptr);
            u32 e0 = entry, x0 = ex, c0 = cn | (ob ? 0x80000000u : 0u);  // the last three results of this lane, newest first
            u32 e1 = 0xFFFFFFFFu, x1 = 0u, c1 = 0u, e2 = 0xFFFFFFFFu, x2 = 0u, c2 = 0u;
            bool settled = false;
            for (u32 sweep = 0; sweep < ALZ_RLH_HUF_SWEEPS; sweep++) {
                const u32 left = wave_bperm((u32)(lane + 63) & 63u, ex);
                const u32 want = lane == 0 ? real : left;
                const bool ch = want != entry;
                if (!wave_ballot(ch)) { settled = true; break; }
                if (ch) {
                    entry = want;
                    if (want == e0) { ex = x0; cn = c0 & 0x7FFFFFFFu; ob = (c0 >> 31) != 0u; }
                    else if (want == e1) { ex = x1; cn = c1 & 0x7FFFFFFFu; ob = (c1 >> 31) != 0u; }
                    else if (want == e2) { ex = x2; cn = c2 & 0x7FFFFFFFu; ob = (c2 >> 31) != 0u; }
                    else {
                        huf20_word<false>(w, entry, tree, tlen, root, ex, cn, ob, nullptr);
                        e2 = e1; x2 = x1; c2 = c1; e1 = e0; x1 = x0; c1 = c0;
                        e0 = entry; x0 = ex; c0 = cn | (ob ? 0x80000000u : 0u);
                    }
                }
            }
            // a round that did not settle, one with an index beyond the tree, and the round the stream ends in: the exact path
            if (!settled || wave_ballot(ob)) break;
            const u32 incl = wave_incl_scan(cn, lane);
            const u32 total = wave_readlane(incl, 63);
            // The round that would complete the output is the exact path's too: the managed loop stops reading at the word that holds the last
            // symbol (:124-130), and a code may be longer than a word (up to 255 bits without a leaf), so the words behind that symbol -- which this
            // round would count as read -- may hold no symbol end at all.  src_used has to stop where the managed Position stops.
            if (total >= symbols - h.i) break;
            huf20_word<true>(w, entry, tree, tlen, root, ex, cn, ob, stage + carry_n + (incl - cn));
            wave_sync();
            const u32 nsym = carry_n + total;                            // symbols staged: stage[0] is symbol h.i - carry_n (an even index in 4-bit mode)
            const u32 nb = NIB ? nsym >> 1 : nsym;                       // whole output bytes
            const u32 ob0 = NIB ? (h.i - carry_n) >> 1 : h.i;            // the first one's index
            const u32 wl = lim > ob0 ? (nb < lim - ob0 ? nb : lim - ob0) : 0u;   // nothing behind min(dst_cap, decom_len) is written
            u8* const o = dst + ob0;
            const u32 a0 = (u32)(reinterpret_cast<uintptr_t>(o) & 15u);
            const u32 ng = wl ? (a0 + wl + 15u) >> 4 : 0u;
            for (u32 g = (u32)lane; g < ng; g += 64u) {                  // one aligned 16-byte granule per lane and pass
                const int k0 = (int)(g << 4) - (int)a0;
                u32 v4[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const int q = k0 + j;
                    if (q >= 0 && (u32)q < wl) {
                        u32 v;
                        if (NIB) {                                       // the 4-bit OR, per output byte: (byte)(treePos << (shift ? 4 : 0)), shift = (i even) ^ little  :145-146
                            const u32 s0 = stage[2 * q], s1 = stage[2 * q + 1];
                            v = little ? (s0 | (s1 << 4)) & 0xFFu : ((s0 << 4) | s1) & 0xFFu;
                        } else v = stage[q];
                        v4[j >> 2] |= v << (8 * (j & 3));
                    }
                }
                if (k0 >= 0 && (u32)(k0 + 16) <= wl) *reinterpret_cast<uint4*>(o + k0) = make_uint4(v4[0], v4[1], v4[2], v4[3]);
                else {
#pragma unroll
                    for (int j = 0; j < 16; j++)
                        if (k0 + j >= 0 && (u32)(k0 + j) < wl) o[k0 + j] = (u8)(v4[j >> 2] >> (8 * (j & 3)));
                }
            }
            u32 keep = 0u;
            if (NIB && (nsym & 1u)) keep = uni((u32)stage[nsym - 1u]);   // an odd symbol waits for its partner
            wave_sync();
            if (NIB && (nsym & 1u)) { if (lane == 0) stage[0] = (u8)keep; carry_n = 1u; } else carry_n = 0u;
            wave_sync();
            const u32 last = wave_readlane(ex, 63);
            h.pos = last & 0xFFu; h.nxt = last >> 8; h.p += 256u; h.i += total;
        }
        const u32 carry = carry_n ? uni((u32)stage[0]) : 0u;
        huf20_exact_tail<NIB>(src, n, lds, tree, tlen, root, h, symbols, dst, lim, little, lane, carry);
    }
    huf20_finish(&results[sid], lane, h, hdr_ok, n, size, cap);
}

// ------------------------------------------------------------------------------------------------ launchers
#define ALZ_RLH_GRID(count) dim3(((count) + ALZ_RLH_WPB - 1) / ALZ_RLH_WPB), dim3(64 * ALZ_RLH_WPB), 0, stream

bool alz_rlh_has_production(int fmt, bool encode) { return !encode && fmt >= 0 && fmt < ALZ_RLH_COUNT; }

hipError_t alz_launch_rlhudson_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                      u32 count, alz_result* results, bool exact) {
    if (count == 0) return hipSuccess;
    if (exact) hipLaunchKernelGGL(alz_rlh_hudson_decode_exact_kernel, ALZ_RLH_GRID(count), (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    else hipLaunchKernelGGL(alz_rlh_hudson_decode_kernel, ALZ_RLH_GRID(count), (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}

hipError_t alz_launch_rlhudson_encode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                      u32 count, alz_result* results) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_rlh_hudson_encode_kernel, ALZ_RLH_GRID(count), (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}

hipError_t alz_launch_rlh_decode(int fmt, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                 u32 count, alz_result* results, bool exact) {
    if (count == 0) return hipSuccess;
    const u8* s = (const u8*)d_src; u8* d = (u8*)d_dst;
    switch (fmt) {
    case ALZ_RLH_RLE30:
        if (exact) hipLaunchKernelGGL(alz_rlh_rle30_decode_exact_kernel, ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        else hipLaunchKernelGGL(alz_rlh_rle30_decode_kernel, ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        break;
    case ALZ_RLH_HUF20_4:
        if (exact) hipLaunchKernelGGL((alz_rlh_huf20_decode_exact_kernel<true>), ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        else hipLaunchKernelGGL((alz_rlh_huf20_decode_kernel<true>), ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        break;
    case ALZ_RLH_HUF20_8:
        if (exact) hipLaunchKernelGGL((alz_rlh_huf20_decode_exact_kernel<false>), ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        else hipLaunchKernelGGL((alz_rlh_huf20_decode_kernel<false>), ALZ_RLH_GRID(count), s, d, streams, index, count, results);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t alz_launch_rlh_encode(int fmt, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                 u32 count, alz_result* results, bool exact) {
    (void)exact;                                                         // one kernel serves both families
    if (count == 0) return hipSuccess;
    if (fmt != ALZ_RLH_RLE30) return hipErrorInvalidValue;
    hipLaunchKernelGGL(alz_rlh_rle30_encode_kernel, ALZ_RLH_GRID(count), (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}
