// alz_bitlz.hip -- gfx950 kernels of CRILAYLA (CRI/CRILAYLA.cs) and ALLZ (Specialized/ALLZ.cs), the two LZ bodies of the reference's
// .Extended assembly that read their tokens bit by bit.  A family of its own beside decode / encode / measure / rlh / aplib
// (tools/kernel_hash.py "bitlz"): neither is an alz_format -- no body in the CPU oracle -- so they have their own entry points
// (alz_bitlz_decode_batch, stream.format = alz_bitlz_kind).  Decode only.
// Citations are relative to the reference's src/AuroraLib.Compression-Extended (CRI/CRILAYLA.cs, Specialized/ALLZ.cs) and
// src/AuroraLib.Compression (IO/FlagReader.cs).
//
// Grid mapping: one wavefront (= one 64-thread workgroup) per stream.  Control flow is wave-uniform: the parse state lives in SGPRs,
// the 64 lanes share the byte work.  Each format has ONE kernel, the exact one: every token is executed as it is parsed.
//
// ALLZ (ALLZ.DecompressHeaderless, ALLZ.cs:90-127) runs on the shared input cache, output window and sink interface of the LZ kernels
// (alz_decode_fast.h, included as it is).  FlagReader(source, Endian.Little): 8-bit flag bytes, LSB first, fetched LAZILY at the current
// input position when a bit is needed and none is left (FlagReader.cs:53-65) -- flag bytes and the raw bytes of literal runs interleave,
// and bits left in a flag byte stay valid across a run.  While produced < decom_len:
//   bit 0: run = ReadALFlag(len_bits) + 1 raw bytes follow at the input position          bit 1: no run
//   then, if still produced < decom_len: distance = ReadALFlag(dist_bits) + 1, length = ReadALFlag(copy_bits) + 3, byte-wise copy.
// ReadALFlag(s): bits = s + (number of 1-bits in front of the first 0-bit); `bits` bits, least significant first; + ((1 << (bits - s)) - 1) << s.
// All of it in C# int arithmetic: computed in u32 (shift counts mod 32, `1 << i` of ReadInt too), read as i32.
//   run < 0                      BAD_TOKEN                          run == 0 / match length <= 0      copies nothing, no error
//   match, length > 0, distance <= 0 or > produced                  BAD_TOKEN, src_used just behind the length field
//   a run or match that passes min(decom_len, dst_cap)              clipped there: OUTPUT_CAPACITY when dst_cap < decom_len, else OUTPUT_SIZE_MISMATCH
//   a flag byte that is missing; a run (after clipping) longer than the input     INPUT_TRUNCATED, src_used = src_len (the bytes that exist are copied)
//   success                      produced == decom_len; src_used = the input position
// The window is the whole output so far: ALZ_ALLZ_LW bytes of it stay in LDS, older sources come back from the stream's own output in HBM
// (OutWin<true>).
//
// CRILAYLA (CRILAYLA.DecompressHeaderless, CRILAYLA.cs:123-188) is read from the LAST input byte down (bits MSB first within a byte, values
// MSB first across bytes) and written from the LAST byte of the destination span down: output byte q goes to dst_off + dst_cap - 1 - q.
// Neither direction exists in the shared headers, so the input cache (CriIn) and the output window (CriWin) are here.  The window keeps the
// ring indexed by the byte's ADDRESS, so that a flush block leaves in aligned 16 B per lane stores exactly as OutWin's does.  Tokens while unread input
// bytes remain (bits left in the last loaded byte are padding):
//   0 + 8 bits                 literal
//   1 + 13 bits + VLE          match: distance = field + 3 (3..8194), length = 3 + fields of 2, 3, 5, 8, 8, ... bits, an all-ones field continues
//   distance > produced        BAD_TOKEN (the length code is read first), src_used = bytes loaded so far
//   does not fit dst_cap       clipped: OUTPUT_CAPACITY, dst_len = dst_cap              input ends inside a token: INPUT_TRUNCATED, src_used = src_len
// 4 KiB of the window stay in LDS, sources older than the ring are read back from the stream's own output in HBM: measured faster than a
// 16 KiB ring that holds the whole window (docs/EXPERIMENTS.md 14).
//
// Every loop consumes input bits or produces output bytes, so its trip count is bounded by src_len or dst_cap; malformed input ends in a status.
#include <hip/hip_runtime.h>

#include "alz_decode_fast.h"
#include "alz_bitlz.h"

#define ALZ_BITLZ_QCH 512u               /* input-cache chunk of both kernels */
#define ALZ_ALLZ_CACHE (2u * ALZ_BITLZ_QCH + 32u)
#define ALZ_ALLZ_LW 4096u                /* LDS ring of the ALLZ kernel */
#define ALZ_CRILAYLA_LW 4096u            /* LDS ring of the CRILAYLA kernel (docs/EXPERIMENTS.md 14: 4 KiB against 16 KiB) */

__device__ __forceinline__ void bitlz_write(alz_result* r, int lane, u32 dst_len, u32 src_used, int status, u32 src_len) {
    if (status == ALZ_ST_INPUT_TRUNCATED) src_used = src_len;
    if (lane == 0) { r->dst_len = dst_len; r->src_used = src_used; r->status = status; r->reserved = 0; }
}

// ------------------------------------------------------------------------------------------------ ALLZ
template <class SK>
__device__ __forceinline__ bool al_fetch(InCache& in, SK& sk, DecState& s, u32 src_len) {           // ReadNextFlag  FlagReader.cs:55-59
    if (s.p >= src_len) { s.eof = true; return false; }
    sk.ensure(in, s.p, 1);
    s.flag = in.peek1(s.p); s.p++; s.bits = 8;
    return true;
}
template <class SK>
__device__ __forceinline__ bool al_bit(InCache& in, SK& sk, DecState& s, u32 src_len, u32& bit) {   // Readbit, LSB first  FlagReader.cs:53-65
    if (s.bits == 0 && !al_fetch(in, sk, s, src_len)) return false;
    bit = (s.flag >> (8u - s.bits)) & 1u;
    s.bits--;
    return true;
}
// ReadALFlag  ALLZ.cs:118-126.  The bits of one flag byte are taken together: a round of either loop consumes at least one input bit.
template <class SK>
__device__ __forceinline__ bool al_flag(InCache& in, SK& sk, DecState& s, u32 src_len, u32 sb, u32& value) {
    u32 bits = sb;
    for (;;) {                                                               // while (flag.Readbit()) bits++;
        if (s.bits == 0 && !al_fetch(in, sk, s, src_len)) return false;
        const u32 avail = s.flag >> (8u - s.bits);                           // the s.bits unread bits, next one lowest; zero above them
        const u32 ones = (u32)__builtin_ctz(~avail);
        if (ones < s.bits) { bits += ones; s.bits -= ones + 1u; break; }
        bits += s.bits; s.bits = 0;
    }
    u32 v = 0;
    const int32_t nb = (int32_t)bits;
    for (int32_t i = 0; i < nb;) {                                           // ReadInt(bits): vaule |= 1 << i  FlagReader.cs:80-86
        if (s.bits == 0 && !al_fetch(in, sk, s, src_len)) return false;
        const u32 left = (u32)(nb - i), take = s.bits < left ? s.bits : left;
        const u32 chunk = (s.flag >> (8u - s.bits)) & ((1u << take) - 1u);
        const u64 c = (u64)chunk << ((u32)i & 31u);                          // (`1 << i` takes i mod 32: bits 32.. land on bits 0.. again)
        v |= (u32)c | (u32)(c >> 32);
        s.bits -= take; i += (int32_t)take;
    }
    value = v + (((1u << ((bits - sb) & 31u)) - 1u) << (sb & 31u));          // :124
    return true;
}

// ALLZ.DecompressHeaderless  ALLZ.cs:90-127.  `lim` = min(decom_len, dst_cap) is the sink's capacity.
template <class SK>
__device__ __forceinline__ void dec_allz_serial(InCache& in, SK& sk, DecState& s, u32 src_len, u32 decom_len, u32 lim,
                                                u32 copy_bits, u32 dist_bits, u32 len_bits) {
    while (sk.produced() < decom_len) {                                      // :95
        u32 bit, v;
        if (!al_bit(in, sk, s, src_len, bit)) return;
        if (!bit) {                                                          // :97-102
            if (!al_flag(in, sk, s, src_len, len_bits, v)) return;
            const int32_t run = (int32_t)(v + 1u);
            if (run < 0) { s.bad = true; return; }                           // destination.Slice(.., negative)
            if (run > 0) {
                const u32 room = lim - sk.produced(), want = (u32)run < room ? (u32)run : room, have = src_len - s.p;
                if (have < want) { (void)sk.run(in, s.p, (u64)have); s.p = src_len; s.eof = true; return; }
                if (!sk.run(in, s.p, (u64)(u32)run)) return;                 // (clipped: the sink sets ovf)
                s.p += (u32)run;
            }
        }
        if (sk.produced() >= decom_len) return;                              // :104
        u32 dv, lv;
        if (!al_flag(in, sk, s, src_len, dist_bits, dv)) return;             // :106
        if (!al_flag(in, sk, s, src_len, copy_bits, lv)) return;             // :107
        const int32_t dist = (int32_t)(dv + 1u), length = (int32_t)(lv + 3u);
        if (length <= 0) continue;                                           // while (length-- > 0)
        if (dist <= 0 || (u32)dist > sk.produced()) { s.bad = true; return; }   // destination[destinationPointer - distance]
        if (!sk.match((u32)dist, (u64)(u32)length, 0u)) return;
    }
}

__global__ __launch_bounds__(64) void alz_bitlz_allz_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                            const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                            u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds[ALZ_ALLZ_LW + ALZ_ALLZ_CACHE];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap), decom = uni(st.decom_len), aux = uni(st.aux0);
    const u32 lim = cap < decom ? cap : decom;
    typedef OutWin<true> OW;
    OW out; out.init(dst_base + st.dst_off, lim, lds, ALZ_ALLZ_LW, lane);
    InCache in; in.init(src_base + st.src_off, src_len, lds + ALZ_ALLZ_LW, lane, ALZ_BITLZ_QCH);
    DecState s; dec_state_init(s);
    DirectSink<OW> sk(out, s);
    dec_allz_serial(in, sk, s, src_len, decom, lim, aux & 0xFFu, (aux >> 8) & 0xFFu, (aux >> 16) & 0xFFu);
    out.finish();
    const int status = s.eof ? ALZ_ST_INPUT_TRUNCATED : s.bad ? ALZ_ST_BAD_TOKEN
                     : s.ovf ? (cap < decom ? ALZ_ST_OUTPUT_CAPACITY : ALZ_ST_OUTPUT_SIZE_MISMATCH) : ALZ_ST_OK;
    bitlz_write(&results[sid], lane, out.produced, s.p, status, src_len);
}

// ------------------------------------------------------------------------------------------------ CRILAYLA
// The compressed bytes from the last one down: ONE chunk of the input in LDS (a token never needs more than the next byte), the chunk
// below it prefetched in registers.  Coordinates as InCache's: a = p + (address of src & 15), chunks aligned in LDS and HBM; loads are
// aligned 8 B granules that overlap [src, src + len).
struct CriIn {
    const u8* gbase; u8* lds; u32 lo, hi, cb; uint2 pf; int lane;
    __device__ __forceinline__ uint2 load_chunk(u32 ca) const {
        uint2 v = make_uint2(0, 0);
        const u32 ga = ca + 8u * (u32)lane;
        if (ga + 8u > lo && ga < hi) v = *reinterpret_cast<const uint2*>(gbase + ga);
        return v;
    }
    __device__ __forceinline__ void init(const u8* src, u32 len, u8* lds_, int lane_) {
        const u32 ishift = (u32)(reinterpret_cast<uintptr_t>(src) & 15u);
        gbase = src - ishift; lds = lds_; lo = ishift; hi = ishift + len; lane = lane_; cb = 0; pf = make_uint2(0, 0);
        if (len == 0) return;
        cb = (hi - 1u) & ~(ALZ_BITLZ_QCH - 1u);
        const uint2 c0 = load_chunk(cb);
        if (cb) pf = load_chunk(cb - ALZ_BITLZ_QCH);
        *reinterpret_cast<uint2*>(lds + 8 * lane) = c0;
        wave_sync();
    }
    // the byte at input offset p (wave-uniform; p goes down by one from call to call)
    __device__ __forceinline__ u32 byte(u32 p) {
        const u32 a = p + lo;
        if (a < cb) {
            wave_sync();
            *reinterpret_cast<uint2*>(lds + 8 * lane) = pf;
            cb -= ALZ_BITLZ_QCH;
            pf = cb ? load_chunk(cb - ALZ_BITLZ_QCH) : make_uint2(0, 0);
            wave_sync();
        }
        return uni((u32)lds[a - cb]);
    }
};

// The output window written DOWN: output byte q lives at base[cap - 1 - q].  Everything is counted in q as in OutWin (produced, flushed,
// pieces of at most a flush block, period doubling); only slot() and the addresses differ: the ring is indexed by the byte's address
// (x + oshift, x = cap - 1 - q, oshift = address of base & 15), so a 16 B granule of the ring is a 16 B granule of HBM and flush blocks
// are aligned blocks of addresses.  Sources older than the ring are read back from the stream's own output.
struct CriWin {
    u8* base; u8* win; u32 lw_mask, fl, oshift, cap, produced, flushed; int lane;
    __device__ __forceinline__ void init(u8* base_, u32 cap_, u8* win_, u32 lw, int lane_) {
        base = base_; cap = cap_; win = win_; lw_mask = lw - 1u; lane = lane_; fl = 1024u;
        oshift = (u32)(reinterpret_cast<uintptr_t>(base_) & 15u);
        produced = 0; flushed = 0;                                           // (no source lies in front of the stream: the ring needs no zeros)
    }
    __device__ __forceinline__ u32 slot(u32 q) const { return (cap - 1u - q + oshift) & lw_mask; }
    // store outputs [flushed, limit) = addresses base + [cap - limit, cap - flushed); 16 B granules aligned in LDS and HBM, ragged ends bytewise
    __device__ void flush_to(u32 limit) {
        wave_sync();
        const u32 a0 = cap - limit + oshift, a1 = cap - flushed + oshift;
        u8* gb = base - oshift;
        for (u32 g = (a0 & ~15u) + 16u * (u32)lane; g < a1; g += 16u * ALZ_WAVE) {
            if (g >= a0 && g + 16u <= a1) {
                const uint4 v = *reinterpret_cast<const uint4*>(win + (g & lw_mask));
                *reinterpret_cast<uint4*>(gb + g) = v;
            } else {
                const u32 b0 = g < a0 ? a0 : g, b1 = g + 16u < a1 ? g + 16u : a1;
                for (u32 b = b0; b < b1; b++) gb[b] = win[b & lw_mask];
            }
        }
        flushed = limit;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");               // stores reach L2 before read-back
    }
    // flush every complete block (of addresses); keeps produced - flushed < fl
    __device__ __forceinline__ void flush_blocks() {
        const u32 lim = (cap - produced + oshift + fl - 1u) & ~(fl - 1u);
        if (lim < cap - flushed + oshift) flush_to(cap + oshift - lim);
    }
    __device__ __forceinline__ void finish() { if (produced > flushed) flush_to(produced); }
    __device__ __forceinline__ void put_byte(u32 b) {
        if (lane == 0) win[slot(produced)] = (u8)b;
        produced += 1;
        if (((cap - produced + oshift) & (fl - 1u)) == 0) flush_blocks();
    }
    // out[q] = out[q - d] for len bytes (d <= produced, len clipped against cap): OutWin::back_copy in this window's coordinates
    __device__ void back_copy(u32 d, u32 len) {
        const u32 lw = lw_mask + 1u;
        u32 done = 0, P = d;                                                 // P: multiple of d, P <= done + d
        while (done < len) {
            u32 span = len - done; if (span > P) span = P;
            u32 off = 0;
            while (off < span) {                                             // pieces of <= fl bytes: unflushed data is never overwritten
                u32 n = span - off; if (n > fl) n = fl;
                const u32 c = produced;
                for (u32 j = (u32)lane; j < n; j += ALZ_WAVE) {
                    const u32 q = c + j, sp = q - P;
                    u32 v;
                    // slots of [c - lw, c + n - lw) are overwritten during this piece: those sources are flushed (n + fl <= lw)
                    if (sp + lw < c + n) v = (u32)__hip_atomic_load(base + (cap - 1u - sp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else v = win[slot(sp)];
                    win[slot(q)] = (u8)v;
                }
                wave_sync();
                produced = c + n; off += n;
                flush_blocks();
            }
            done += span;
            if (span == P) P *= 2u;
        }
    }
};

struct CriBits { u32 rem, flag, bits; };                                     // unread input bytes (sourcePointer + 1), bitBuffer, bitsLeft

// GetBits  CRILAYLA.cs:165-188; false: the input ended inside the field
__device__ __forceinline__ bool cri_get(CriIn& in, CriBits& b, u32 n, u32& v) {
    v = 0;
    while (n) {
        if (b.bits == 0) {
            if (b.rem == 0) return false;                                    // input[-1]
            b.rem--; b.flag = in.byte(b.rem); b.bits = 8;
        }
        const u32 take = b.bits < n ? b.bits : n;
        v = (v << take) | ((b.flag >> (b.bits - take)) & ((1u << take) - 1u));
        b.bits -= take; n -= take;
    }
    return true;
}

// CRILAYLA.DecompressHeaderless  CRILAYLA.cs:123-163; returns the status
template <class OW>
__device__ __forceinline__ int dec_crilayla(CriIn& in, OW& out, CriBits& b) {
    while (b.rem > 0) {                                                      // :132
        u32 t, f;
        if (!cri_get(in, b, 1u, t)) return ALZ_ST_INPUT_TRUNCATED;
        if (t) {
            if (!cri_get(in, b, 13u, f)) return ALZ_ST_INPUT_TRUNCATED;
            const u32 dist = f + 3u;                                         // :136
            u64 length = 3;
            for (u32 lvl = 0;;) {                                            // :140-148: every round reads at least two input bits
                const u32 nb = lvl == 0u ? 2u : (lvl == 1u ? 3u : (lvl == 2u ? 5u : 8u));
                if (!cri_get(in, b, nb, f)) return ALZ_ST_INPUT_TRUNCATED;
                length += f;
                if (f != (1u << nb) - 1u) break;
                if (lvl != 3u) lvl++;
            }
            if (dist > out.produced) return ALZ_ST_BAD_TOKEN;                // destination[destinationPointer + distance] beyond the span
            const u32 room = out.cap - out.produced;
            out.back_copy(dist, length > (u64)room ? room : (u32)length);
            if (length > (u64)room) return ALZ_ST_OUTPUT_CAPACITY;
        } else {
            if (!cri_get(in, b, 8u, f)) return ALZ_ST_INPUT_TRUNCATED;
            if (out.produced >= out.cap) return ALZ_ST_OUTPUT_CAPACITY;
            out.put_byte(f);                                                 // :158
        }
    }
    return ALZ_ST_OK;
}

__global__ __launch_bounds__(64) void alz_bitlz_crilayla_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                                const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                                u32 count, alz_result* __restrict__ results) {
    constexpr u32 LW = ALZ_CRILAYLA_LW;
    static_assert(LW >= 4096u && (LW & (LW - 1u)) == 0u, "the ring is a power of two of at least four flush blocks");
    __shared__ __attribute__((aligned(16))) u8 lds[LW + ALZ_BITLZ_QCH];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    CriWin out; out.init(dst_base + st.dst_off, cap, lds, LW, lane);
    CriIn in; in.init(src_base + st.src_off, src_len, lds + LW, lane);
    CriBits b; b.rem = src_len; b.flag = 0; b.bits = 0;
    const int status = dec_crilayla(in, out, b);
    out.finish();
    bitlz_write(&results[sid], lane, out.produced, src_len - b.rem, status, src_len);
}

// ------------------------------------------------------------------------------------------------ launcher
hipError_t alz_launch_bitlz_decode(int kind, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                   u32 count, alz_result* results) {
    if (count == 0) return hipSuccess;
    if (kind == ALZ_BITLZ_ALLZ)
        hipLaunchKernelGGL(alz_bitlz_allz_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    else
        hipLaunchKernelGGL(alz_bitlz_crilayla_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}
