// alz_aplib.hip -- gfx950 kernels of aPLib (Formats/Common/aPLib.cs), the last LzWindows user of the reference.
// A family of its own beside decode / encode / measure / rlh (tools/kernel_hash.py "aplib"): aPLib is no alz_format -- its body carries
// no size, its window is 2 MiB and it has no body in the CPU oracle -- so it has its own entry points (alz_aplib_*).  It shares the input
// cache, the output window, the sink interface and the chunked byte phase with the LZ kernels (alz_decode_fast.h, included as it is).
// Citations are relative to the reference's src/AuroraLib.Compression (Formats/Common/aPLib.cs, IO/FlagReader.cs, IO/LzWindows.cs).
//
// Grid mapping: one wavefront (= one 64-thread workgroup) per stream.  Control flow is wave-uniform: the parse state lives in SGPRs,
// the 64 lanes share the byte work.
//
// The grammar (aPLib.DecompressHeaderless, aPLib.cs:105-181).  The first byte is a literal.  Then tokens, each introduced by a prefix of
// up to three 1-bits read from a FlagReader(source, Endian.Big): 8-bit flag bytes, MSB first, fetched LAZILY at the current input position
// when a bit is needed and none is left (FlagReader.cs:53-65) -- flag bytes and data bytes interleave in one stream:
//   0     literal: the next byte                                                           lwm = false
//   10    gamma g.  !lwm && g == 2: repeat -- distance = lastOffset, length = gamma.
//         otherwise distance = ((g - (lwm ? 2 : 3)) << 8) | next byte, length = gamma + LengthDelta(distance); lastOffset = distance.
//                                                                                          lwm = true
//   110   byte b: distance = b >> 1, length = 2 + (b & 1); distance 0 ENDS the stream; lastOffset = distance    lwm = true
//   111   4 bits o: o > 0 copies one byte from distance o, o == 0 writes 0x00               lwm = false
// gamma: v = 1; do { v = v << 1 | bit } while (bit);   LengthDelta(d): d < 0x80 || d >= 0x7D00 -> 2, d >= 0x500 -> 1, else 0.
//
// Frozen edge rules:
//   32-bit arithmetic  ReadGamma and (offset << 8) | byte are C# ints in an unchecked context: computed in u32, read as i32.  The repeat
//                      test g == 2 uses the wrapped value.
//   distance           negative as i32, or larger than W = 0x200000: ALZ_ST_BAD_TOKEN (E3).  The length gamma behind it is read first (the
//                      managed code reads it before BackCopy): src_used is just behind that gamma, and input that ends inside it is
//                      INPUT_TRUNCATED.
//   length             after LengthDelta, as i32: <= 0 copies nothing (LzWindows.cs:80) -- lastOffset and lwm are still updated; anything
//                      positive is legal and clipped by dst_cap (E5).
//   distance 0         (repeat before any match: lastOffset starts at 0; a normal match with high part 0 and low byte 0) copies from W
//                      back (E1); sources in front of the stream start read 0x00 (E2).
//   end of input       a flag byte or data byte that is missing: INPUT_TRUNCATED, dst_len = what was produced, src_used = src_len.
//                      Empty input: INPUT_TRUNCATED, dst_len 0.
//   capacity           a literal or match that does not fit dst_cap is clipped: OUTPUT_CAPACITY, dst_len = dst_cap, src_used unspecified.
//   success            OK means the end marker was read; src_used is just behind its byte.  decom_len, aux0, aux1, format are ignored.
//
// Three kernels around the one parser (dec_aplib_serial<SK>):
//   exact       DirectSink<OutWin<true>>: every token executed as it is parsed -- the reference semantics (alz_ctx_set_exact_kernels).
//   production  the parser on the scalar path records tokens into a 64-entry queue in lane registers (ApQueueSink); the chunked byte
//               phase of alz_emit_chunk.h executes a queue at a time.  ALZ_APLIB_LW bytes of the window stay in LDS, older sources
//               come back from the stream's own output in HBM; write-back is coalesced at 16 B per lane (OutWin::flush_to).  The parser
//               is resumable at token boundaries, so the byte phase is inlined once, in the kernel's loop.  The queue takes tokens of
//               any length (one above 1 KiB runs alone in the byte phase) and cuts the one that meets dst_cap itself (E5).  A match whose
//               distance is above 0x1FFFF -- the 17-bit distance field of the byte phase's descriptor and token table -- drains the
//               queue and is copied straight from HBM (ap_far_copy), as QueueSink does for RefPack's longest distances.
//   measure     the parser on a counting sink: reads the input, writes nothing but the result.
#include <hip/hip_runtime.h>

#include "alz_decode_fast.h"
#include "alz_aplib.h"

#ifndef ALZ_APLIB_LW
#define ALZ_APLIB_LW 4096u               /* LDS ring of the production kernel (docs/EXPERIMENTS.md: 4 KiB against 16 KiB) */
#endif
// The rule (docs/EXPERIMENTS.md 13): the token-queue kernel is the default only if it is MEASURED faster than the exact kernel on the
// 10 000 x 256 KiB batch of tools/bench_aplib.py; until then, and otherwise, the default is the exact kernel.
#ifndef ALZ_APLIB_DEFAULT_IS_PRODUCTION
#define ALZ_APLIB_DEFAULT_IS_PRODUCTION 0
#endif
#define ALZ_APLIB_QCH 512u               /* input-cache chunk: two of them + 32 guard bytes per wavefront */
#define ALZ_APLIB_CACHE (2u * ALZ_APLIB_QCH + 32u)
#define ALZ_APLIB_MAXDIST 0x1FFFFu       /* ALZ_DESC_DIST: what the byte phase's descriptor and token table hold */

// what crosses tokens beside DecState (p, bits, flag): aPLib.cs:107-108, and whether the first literal is out
struct ApState { u32 last; bool lwm, started; };
__device__ __forceinline__ void ap_state_init(ApState& a) { a.last = 0; a.lwm = false; a.started = false; }

template <class SK>
__device__ __forceinline__ bool ap_byte(InCache& in, SK& sk, DecState& s, u32 src_len, u32& b) {   // source.ReadUInt8()
    if (s.p >= src_len) { s.eof = true; return false; }
    sk.ensure(in, s.p, 1);
    b = in.peek1(s.p); s.p++;
    return true;
}
template <class SK>
__device__ __forceinline__ bool ap_bit(InCache& in, SK& sk, DecState& s, u32 src_len, u32& bit) {  // FlagReader.Readbit  FlagReader.cs:53-65
    if (s.bits == 0) { u32 f; if (!ap_byte(in, sk, s, src_len, f)) return false; s.flag = f; s.bits = 8; }
    s.bits--;
    bit = (s.flag >> s.bits) & 1u;
    return true;
}
template <class SK>
__device__ __forceinline__ bool ap_gamma(InCache& in, SK& sk, DecState& s, u32 src_len, u32& v) {  // ReadGamma  aPLib.cs:297-307 (wraps as the int does)
    v = 1u;
    u32 b, more;
    do {
        if (!ap_bit(in, sk, s, src_len, b)) return false;
        v = (v << 1) | b;
        if (!ap_bit(in, sk, s, src_len, more)) return false;
    } while (more);
    return true;
}
__device__ __forceinline__ u32 ap_length_delta(u32 d) {                                            // LengthDelta  aPLib.cs:288-295 (d >= 0 here)
    return (d < 0x80u || d >= 0x7D00u) ? 2u : (d >= 0x500u ? 1u : 0u);
}

// aPLib.DecompressHeaderless  Formats/Common/aPLib.cs:105-181.  Resumable at token boundaries: everything a token changes (s, a) is
// final before the sink sees it, so a sink may answer false for "come back later" (ApQueueSink) as well as for E5.
template <class SK>
__device__ __forceinline__ void dec_aplib_serial(InCache& in, SK& sk, DecState& s, u32 src_len, ApState& a) {
    const u32 W = ALZ_APLIB_WINDOW;
    for (;;) {
        // what the token turns out to be: one byte `b` to write (length == 0), or a copy of `length` bytes from `d`.  The sink is called in
        // ONE place behind the branches (one inlined copy of the window code instead of four).
        u32 prefix = 0, bit, b = 0, d = 0;
        int32_t length = 0;
        bool copy = false;
        if (a.started) {                                                     // :116-118
            do {
                if (!ap_bit(in, sk, s, src_len, bit)) return;
                prefix += bit;
            } while (bit && prefix < 3u);
        } else a.started = true;                                             // buffer.WriteByte(source.ReadUInt8())  :113: the literal branch without its flag bit (lwm is false)
        if (prefix == 0u) {                                                  // literal  :122-125
            if (!ap_byte(in, sk, s, src_len, b)) return;
            a.lwm = false;
        } else if (prefix == 1u) {                                           // :126-149
            u32 g, lg;
            if (!ap_gamma(in, sk, s, src_len, g)) return;
            if (!a.lwm && g == 2u) {                                         // repeat last offset  :130-136
                d = a.last;
                if (!ap_gamma(in, sk, s, src_len, lg)) return;
                length = (int32_t)lg;
            } else {
                u32 lo;
                const u32 hi = g - (a.lwm ? 2u : 3u);                        // :139
                if (!ap_byte(in, sk, s, src_len, lo)) return;
                d = (hi << 8) | lo;                                          // :140
                if (!ap_gamma(in, sk, s, src_len, lg)) return;               // :141 (read before BackCopy sees the distance)
                if ((int32_t)d < 0 || d > W) { s.bad = true; return; }       // E3
                length = (int32_t)(lg + ap_length_delta(d));                 // :142
                a.last = d;                                                  // :145
            }
            a.lwm = true;                                                    // :147
            if (length <= 0) continue;                                       // LzWindows.cs:80: copies nothing
            copy = true;
        } else if (prefix == 2u) {                                           // :151-165
            if (!ap_byte(in, sk, s, src_len, b)) return;
            d = b >> 1; length = (int32_t)(2u + (b & 1u));
            if (d == 0u) { s.done = true; return; }                          // end  :157-158
            a.last = d; a.lwm = true;
            copy = true;
        } else {                                                             // :167-178
            for (int i = 0; i < 4; i++) { if (!ap_bit(in, sk, s, src_len, bit)) return; d = (d << 1) | bit; }   // ReadInt(4, true)
            a.lwm = false;
            length = 1; copy = d != 0u;                                      // offset 0: WriteByte(0)
        }
        if (copy) { if (!sk.match(d, (u64)(u32)length, W)) return; }
        else if (!sk.lit(b)) return;
    }
}

__device__ __forceinline__ int ap_status(const DecState& s) {
    if (s.eof) return ALZ_ST_INPUT_TRUNCATED;
    if (s.bad) return ALZ_ST_BAD_TOKEN;
    if (s.ovf) return ALZ_ST_OUTPUT_CAPACITY;
    return ALZ_ST_OK;                                                        // (s.done: the end marker was read)
}
__device__ __forceinline__ void ap_write(alz_result* r, int lane, u32 dst_len, u32 src_used, int status, u32 src_len) {
    if (status == ALZ_ST_INPUT_TRUNCATED) src_used = src_len;
    if (lane == 0) { r->dst_len = dst_len; r->src_used = src_used; r->status = status; r->reserved = 0; }
}

// ------------------------------------------------------------------------------------------------ exact
#define ALZ_APLIB_EXACT_LW 4096u
__global__ __launch_bounds__(64) void alz_aplib_decode_exact_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                                    const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                                    u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds[ALZ_APLIB_EXACT_LW + ALZ_APLIB_CACHE];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    typedef OutWin<true> OW;
    OW out; out.init(dst_base + st.dst_off, cap, lds, ALZ_APLIB_EXACT_LW, lane);
    InCache in; in.init(src_base + st.src_off, src_len, lds + ALZ_APLIB_EXACT_LW, lane, ALZ_APLIB_QCH);
    DecState s; dec_state_init(s);
    ApState a; ap_state_init(a);
    DirectSink<OW> sk(out, s);
    dec_aplib_serial(in, sk, s, src_len, a);
    out.finish();
    ap_write(&results[sid], lane, out.produced, s.p, ap_status(s), src_len);
}

// ------------------------------------------------------------------------------------------------ production
// The token queue: one token per lane in two registers (length, byte-phase descriptor).  The sink never executes anything: it answers
// false when the kernel has to act -- the queue is full, or a token has to go around it (`direct`) -- and the parser, whose state is
// final at that point, is simply entered again.
template <class OW>
struct ApQueueSink {
    OW& out; DecState& s;
    u32 qlen, qdesc;          // per-lane token registers
    u32 nt, qbytes;           // tokens queued, bytes they will produce (wave-uniform)
    bool direct, at_cap;      // a far match to copy behind the queue (ddist, dlen) | a literal that meets dst_cap
    u32 ddist, dlen;
    __device__ __forceinline__ ApQueueSink(OW& o, DecState& st) : out(o), s(st), qlen(0), qdesc(0), nt(0), qbytes(0), direct(false), at_cap(false), ddist(0), dlen(0) {}
    __device__ __forceinline__ u32 produced() const { return out.produced + qbytes; }
    __device__ __forceinline__ void ensure(InCache& in, u32 p, u32 need) { in.ensure(p, need); }   // (no queued token points into the input cache)
    __device__ __forceinline__ bool push(u32 len, u32 desc) {
        qlen = wave_writelane(qlen, uni(len), uni(nt));
        qdesc = wave_writelane(qdesc, uni(desc), uni(nt));
        nt = uni(nt + 1u); qbytes = uni(qbytes + len);
        return nt < 64u && qbytes < 0x40000000u;
    }
    __device__ __forceinline__ bool lit(u32 b) {
        if (produced() >= out.cap) { at_cap = true; return false; }          // E5 at its exact place in the stream
        return push(1u, ALZ_DESC_LIT(b & 0xFFu));
    }
    __device__ __forceinline__ bool match(u32 dist, u64 len, u32 w) {
        if (dist == 0u) dist = w;                                            // E1
        if (dist > ALZ_APLIB_MAXDIST) {
            direct = true; ddist = dist; dlen = (u32)len;                    // (len < 2^31: a positive int)
            return false;
        }
        if (len > (u64)(out.cap - produced())) { len = out.cap - produced(); s.ovf = true; if (len == 0) return false; (void)push((u32)len, ALZ_DESC_MATCH(dist)); return false; }   // E5
        return push((u32)len, ALZ_DESC_MATCH(dist));
    }
    __device__ __forceinline__ bool run(InCache&, u32, u64) { return true; } // (aPLib has no literal runs)
    __device__ __forceinline__ void flush() {}
};

// A match the queue cannot hold: its distance is above ALZ_APLIB_MAXDIST, so every source byte lies far outside the ring -- flushed
// long ago -- and comes back from the stream's own output in HBM (in front of the stream start: 0x00, E2).  Pieces of at most one
// flush block, so that unflushed bytes of the ring are never overwritten; a piece never reads what it writes (len of a piece < d).
template <class OW>
__device__ __forceinline__ void ap_far_copy(OW& out, u32 d, u32 len) {
    out.slack_dirty = true;
    for (u32 done = 0; done < len;) {
        const u32 n = len - done < out.fl ? len - done : out.fl;
        const u32 c = out.produced;
        for (u32 j = (u32)out.lane; j < n; j += ALZ_WAVE) {
            const u32 q = c + j;
            const u32 v = q >= d ? (u32)__hip_atomic_load(out.dst + (q - d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            out.win[out.slot(q)] = (u8)v;
        }
        wave_sync();
        out.produced = c + n; done += n;
        out.flush_blocks();
    }
}

// LDS per wavefront: byte-phase scratch (marks + token table) | input cache | ring + its mirror
__global__ __launch_bounds__(64) void alz_aplib_decode_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                              const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                              u32 count, alz_result* __restrict__ results) {
    constexpr u32 LW = ALZ_APLIB_LW;
    __shared__ __attribute__((aligned(16))) u8 lds[ALZ_EMIT_SCRATCH + ALZ_APLIB_CACHE + LW + ALZ_WIN_SLACK];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    u32 sid = uni(index_list ? index_list[bid] : bid);
    const alz_stream st = streams[sid];
    u32 src_len = uni(st.src_len); const u32 cap = uni(st.dst_cap);
    u8* const scratch = lds;
    u8* const inc_lds = lds + ALZ_EMIT_SCRATCH;
    typedef OutWin<true> OW;
    typedef EmitCfg<LW - 1u, false, false, true> CFG;                        // single literals, sources older than the ring from HBM
    OW out; out.init(dst_base + st.dst_off, cap, inc_lds + ALZ_APLIB_CACHE, LW, lane, ALZ_WIN_SLACK);
    scratch[lane] = 0; scratch[64 + lane] = 0;
    InCache in; in.init(src_base + st.src_off, src_len, inc_lds, lane, ALZ_APLIB_QCH);
    DecState s; dec_state_init(s);
    ApState a; ap_state_init(a);
    ApQueueSink<OW> sk(out, s);
    for (;;) {
        dec_aplib_serial(in, sk, s, src_len, a);
        if (sk.nt) {                                                         // the one copy of the byte phase
            // The byte phase wants most of the scalar registers for itself, and the parser's state is dead weight while it runs: it is parked
            // in the lanes of one VGPR across it (once per queue, where the register allocator would otherwise spill inside the parser's loops).
            u32 pk = 0;
            const u64 gb = (u64)in.gbase;
            const u32 fl = (a.lwm ? 1u : 0u) | (a.started ? 2u : 0u) | (sk.direct ? 4u : 0u) | (sk.at_cap ? 8u : 0u) | (s.eof ? 16u : 0u) | (s.bad ? 32u : 0u) | (s.done ? 64u : 0u) | (s.ovf ? 128u : 0u);
            pk = wave_writelane(pk, s.p, 0u); pk = wave_writelane(pk, s.bits, 1u); pk = wave_writelane(pk, s.flag, 2u); pk = wave_writelane(pk, a.last, 3u);
            pk = wave_writelane(pk, fl, 4u); pk = wave_writelane(pk, sk.ddist, 5u); pk = wave_writelane(pk, sk.dlen, 6u); pk = wave_writelane(pk, in.cb, 7u);
            pk = wave_writelane(pk, in.lo, 8u); pk = wave_writelane(pk, in.hi, 9u); pk = wave_writelane(pk, (u32)gb, 10u); pk = wave_writelane(pk, (u32)(gb >> 32), 11u);
            pk = wave_writelane(pk, src_len, 12u); pk = wave_writelane(pk, sid, 13u);
            DecState es; dec_state_init(es);
            u32 last;
            (void)fast_emit<OW, CFG>(out, es, 0xFFFFFFFFu, lanes_below(sk.nt), sk.qlen, sk.qdesc, 0u, scratch, inc_lds, lane, last, ALZ_APLIB_WINDOW);
            s.p = wave_readlane(pk, 0u); s.bits = wave_readlane(pk, 1u); s.flag = wave_readlane(pk, 2u); a.last = wave_readlane(pk, 3u);
            const u32 f2 = wave_readlane(pk, 4u);
            a.lwm = (f2 & 1u) != 0u; a.started = (f2 & 2u) != 0u; sk.direct = (f2 & 4u) != 0u; sk.at_cap = (f2 & 8u) != 0u;
            s.eof = (f2 & 16u) != 0u; s.bad = (f2 & 32u) != 0u; s.done = (f2 & 64u) != 0u; s.ovf = (f2 & 128u) != 0u || es.ovf;
            sk.ddist = wave_readlane(pk, 5u); sk.dlen = wave_readlane(pk, 6u); in.cb = wave_readlane(pk, 7u);
            in.lo = wave_readlane(pk, 8u); in.hi = wave_readlane(pk, 9u);
            in.gbase = reinterpret_cast<const u8*>(((u64)wave_readlane(pk, 11u) << 32) | wave_readlane(pk, 10u));
            src_len = wave_readlane(pk, 12u); sid = wave_readlane(pk, 13u);
            sk.nt = 0; sk.qbytes = 0;
        }
        if (sk.direct) {
            sk.direct = false;
            ap_far_copy(out, sk.ddist, clip_token(out, s, (u64)sk.dlen));    // E5
        }
        if (sk.at_cap) (void)clip_token(out, s, 1u);
        if (s.eof || s.bad || s.done || s.ovf) break;
    }
    out.finish();
    ap_write(&results[sid], lane, out.produced, s.p, ap_status(s), src_len);
}

// ------------------------------------------------------------------------------------------------ measure
// The counting sink: dst_cap only bounds the count (E5 as the decoder reports it: dst_len = dst_cap).
struct ApCountSink {
    DecState& s; u32 n, cap;
    __device__ __forceinline__ ApCountSink(DecState& st, u32 c) : s(st), n(0), cap(c) {}
    __device__ __forceinline__ u32 produced() const { return n; }
    __device__ __forceinline__ void ensure(InCache& in, u32 p, u32 need) { in.ensure(p, need); }
    __device__ __forceinline__ bool add(u64 len) {
        if (len > (u64)(cap - n)) { s.ovf = true; s.attempted_end = (u64)n + len; n = cap; return false; }
        n += (u32)len;
        return true;
    }
    __device__ __forceinline__ bool lit(u32) { return add(1u); }
    __device__ __forceinline__ bool match(u32, u64 len, u32) { return add(len); }
    __device__ __forceinline__ bool run(InCache&, u32, u64 len) { return add(len); }
    __device__ __forceinline__ void flush() {}
};

__global__ __launch_bounds__(64) void alz_aplib_measure_kernel(const u8* __restrict__ src_base, const alz_stream* __restrict__ streams,
                                                               const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds[ALZ_APLIB_CACHE];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    InCache in; in.init(src_base + st.src_off, src_len, lds, lane, ALZ_APLIB_QCH);
    DecState s; dec_state_init(s);
    ApState a; ap_state_init(a);
    ApCountSink sk(s, cap);
    dec_aplib_serial(in, sk, s, src_len, a);
    ap_write(&results[sid], lane, sk.n, s.p, ap_status(s), src_len);
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t alz_launch_aplib_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                   u32 count, alz_result* results, int family) {
    if (count == 0) return hipSuccess;
    const bool exact = family == ALZ_APLIB_EXACT || (family == ALZ_APLIB_DEFAULT && !ALZ_APLIB_DEFAULT_IS_PRODUCTION);
    if (exact) hipLaunchKernelGGL(alz_aplib_decode_exact_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    else hipLaunchKernelGGL(alz_aplib_decode_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}

hipError_t alz_launch_aplib_measure(hipStream_t stream, const void* d_src, const alz_stream* streams, const u32* index, u32 count, alz_result* results) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_aplib_measure_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, streams, index, count, results);
    return hipGetLastError();
}
