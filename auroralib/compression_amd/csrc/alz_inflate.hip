// alz_inflate.hip -- gfx950 kernels of DEFLATE (RFC 1951), the body of the reference's ZLib and GZip classes (Formats/Common/ZLib.cs,
// GZip.cs) and of the zlib wrappers of its .Extended assembly.  The reference hands these bodies to the BCL (ZLibStream / GZipStream), so
// there is no managed loop to restate: the contract is zlib's `inflate` with window bits -15 and no dictionary.  A family of its own
// beside decode / encode / measure / rlh / aplib / bitlz (tools/kernel_hash.py "inflate"): DEFLATE is no alz_format -- it has its own
// entry points (alz_inflate_*).  It shares the input cache, the output window and the sink interface with the LZ kernels
// (alz_decode_fast.h, included as it is).
//
// Grid mapping: one wavefront (= one 64-thread workgroup) per stream.  Control flow is wave-uniform: the parse state lives in SGPRs,
// the 64 lanes share the byte work (match copies, stored runs, write-back) and the building of the Huffman tables.
//
// ONE parser (dec_inflate_serial<SK>), two kernels around it, each the only one of its kind (every context mode runs them):
//   decode   DirectSink<OutWin<true>>: every symbol is executed as it is parsed.  ALZ_INFLATE_LW bytes of the 32 KiB window stay in LDS,
//            older sources come back from the stream's own output in HBM; write-back is coalesced at 16 B per lane (OutWin::flush_to).
//   measure  the parser on a counting sink: reads the input, writes nothing but the result.
//
// Bit source.  DEFLATE packs bits LSB first: a 64-bit buffer `bb` holds `nb` valid bits, the next one lowest, and is refilled from the
// input cache in whole bytes (up to four at a time) until it holds 48 -- what the longest symbol needs (15 + 5 + 15 + 13) -- or the input
// ends.  Bits above `nb` are zero, so a table lookup past the end of the input still answers with a code; it counts only if its bits
// are all present (code length <= nb), exactly as zlib's "pull a byte until the code resolves" does.
//
// Tables, in LDS, per wavefront.  Huffman codes are stored MSB first, so the tables are indexed by BIT-REVERSED codes: the next 9 bits of
// `bb` index the literal/length table, the next 6 the distance table (zlib's own root sizes).  An entry is (symbol << 4) | code length;
// 0 is a code the set does not have (an incomplete single-code set, an empty distance set); length field 15 marks a code longer than
// the index.  Longer codes are resolved by the CANONICAL arrays -- first code, count and first index into the symbols sorted by
// (length, symbol), per length -- and not by sub-tables: the arrays take 96 + 2 * 288 bytes where zlib's worst-case sub-tables take
// 1.3 KiB more, they are what the lane-parallel build computes anyway (the replicated entries need every symbol's canonical code), and a
// code above 9 bits is rare by construction of a Huffman code (each has probability below 2^-9), so the at most six compares of the slow
// path do not show.  Length and distance bases and extra-bit counts are arithmetic on the symbol (no table).
// A dynamic block's tables are built lane-parallel: the code-length code (19 lengths, one per lane) through the same builder, the
// lengths expanded by a scalar walk (repeat runs 16 / 17 / 18 written by the lanes), then per table: count per length (ballots),
// first codes (a 15-step scalar loop), and every lane writes the replicated entries of its symbols (rank among the symbols of its
// length = ballot + mbcnt).  The fixed tables are built the same way from the fixed lengths, on first use, and again only if a dynamic
// block has overwritten them since.
// LDS: 2 304 bytes of tables + 1 056 of input cache (+ ALZ_INFLATE_LW of window in the decode kernel): 5.3 KiB per wavefront at the
// default 2 KiB ring, 30 wavefronts per CU of 160 KiB.
//
// PROGRESS.  Every loop iteration of the parser either consumes input bits or ends the stream: a block header costs at least 3 bits, a
// stored block at least 32 more, every code-length symbol and every literal/length symbol at least 1 (a lookup that finds no code, or a
// code whose bits are not all present, ends the stream).  The refill loop adds at least one byte per round.  So the trip count of every
// loop is bounded by 8 * src_len, and hostile input cannot spin: it ends in a status.
//
// Frozen semantics (include/auroralz.h).  The order of the tests is zlib's: the bits of a field are needed before
// the field is judged (INPUT_TRUNCATED wins over BAD_TOKEN when the field is cut), a malformed dynamic header is BAD_TOKEN when it is
// parsed, `distance > bytes produced` is tested before the sink sees the match (rule E2 never applies), and a match counts as one symbol:
// its code, extra bits, distance code and distance extra bits are all present or it produces nothing.
#include <hip/hip_runtime.h>

#include "alz_decode_fast.h"
#include "alz_inflate.h"

#ifndef ALZ_INFLATE_LW
#define ALZ_INFLATE_LW 2048u             /* LDS ring of the decode kernel (docs/EXPERIMENTS.md 16) */
#endif
#define ALZ_INFLATE_QCH 512u             /* input-cache chunk: two of them + 32 guard bytes per wavefront */
#define ALZ_INFLATE_CACHE (2u * ALZ_INFLATE_QCH + 32u)

#define INF_LIT_PB 9u                    /* index bits of the literal/length table */
#define INF_DIST_PB 6u                   /* ... of the distance table */
#define INF_CL_PB 7u                     /* ... of the code-length table (its longest code) */
#define INF_LONG 15u                     /* length field of an entry whose code is longer than the index */
// byte offsets inside the table area (16 B aligned).  The code-length code lives where the tables it describes are built afterwards:
// its table in the literal/length table, its canonical arrays and sorted symbols in the distance set's.
#define INF_O_LIT 0u                     /* u16[512] */
#define INF_O_DIST 1024u                 /* u16[64] */
#define INF_O_SLIT 1152u                 /* u16[288]: symbols sorted by (length, symbol) */
#define INF_O_SDIST 1728u                /* u16[32] */
#define INF_O_CLIT 1792u                 /* u16[3][16]: first code, count, first sorted index -- per code length */
#define INF_O_CDIST 1888u
#define INF_O_LENS 1984u                 /* u8[320]: the code lengths of the block being opened */
#define ALZ_INFLATE_TABLES 2304u

struct InfBits { u64 bb; u32 nb; };      // the bit buffer: nb valid bits, the next one lowest, zeros above

template <class SK>
__device__ __forceinline__ void inf_refill(InCache& in, SK& sk, DecState& s, InfBits& b, u32 src_len) {
    while (b.nb < 48u && s.p < src_len) {                                    // (room >= 2 bytes: every round adds at least one)
        u32 take = (64u - b.nb) >> 3;
        if (take > 4u) take = 4u;
        if (take > src_len - s.p) take = src_len - s.p;
        sk.ensure(in, s.p, 4);
        u32 v = in.peek4(s.p);
        if (take < 4u) v &= (1u << (8u * take)) - 1u;                        // (bytes past the input end are unspecified)
        b.bb |= (u64)v << b.nb; b.nb += 8u * take; s.p += take;
    }
}
// n <= 48 bits are present, or the input is truncated
template <class SK>
__device__ __forceinline__ bool inf_need(InCache& in, SK& sk, DecState& s, InfBits& b, u32 src_len, u32 n) {
    if (b.nb < n) {
        inf_refill(in, sk, s, b, src_len);
        if (b.nb < n) { s.eof = true; return false; }
    }
    return true;
}
__device__ __forceinline__ u32 inf_take(InfBits& b, u32 n) {                 // n <= 32 present bits
    const u32 v = (u32)b.bb & (u32)((1ull << n) - 1ull);
    b.bb >>= n; b.nb -= n;
    return v;
}

// One Huffman table from nsym code lengths at t + lens_off: canonical arrays, sorted symbols, the bit-reversed lookup table of 2^pb entries.
// false: the set is over-subscribed, or incomplete where zlib's inflate_table refuses that (`codes`: the code-length code, always;
// otherwise unless its longest code is 1 bit).  A set with no code at all leaves a table of zeros: legal for distances, and what the
// caller makes of it for the code-length code.
__device__ __forceinline__ bool inf_build(u8* t, u32 tab_off, u32 pb, u32 lens_off, u32 nsym, u32 canon_off, u32 sorted_off, bool codes, int lane) {
    asm volatile("" : "+v"(lane));                                           // (the lane predicates below are computed here, not kept in scalar registers from the kernel's entry on)
    u16* const tab = reinterpret_cast<u16*>(t + tab_off);
    u16* const canon = reinterpret_cast<u16*>(t + canon_off);
    u16* const sorted = reinterpret_cast<u16*>(t + sorted_off);
    const u8* const lens = t + lens_off;
    const u32 tsize = 1u << pb;
    wave_sync();
    for (u32 i = 8u * (u32)lane; i < tsize; i += 8u * ALZ_WAVE) *reinterpret_cast<uint4*>(tab + i) = make_uint4(0, 0, 0, 0);
    u32 cnt = 0;                                                             // lane L: the number of codes of length L
    for (u32 base = 0; base < nsym; base += ALZ_WAVE) {
        const u32 sym = base + (u32)lane, l = sym < nsym ? (u32)lens[sym] : 0u;
#pragma unroll 1
        for (u32 L = 1; L <= 15u; L++) {                                     // (rolled: fifteen ballots in flight are thirty scalar registers)
            const u32 c = (u32)__popcll(wave_ballot(l == L));
            cnt += (u32)lane == L ? c : 0u;
        }
    }
    int32_t left = 1;
    u32 code = 0, off = 0, maxl = 0, pk = 0;                                 // pk, lane L: first code | first sorted index << 16
#pragma unroll 1
    for (u32 L = 1; L <= 15u; L++) {
        const u32 c = wave_readlane(cnt, L);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return false;                                          // over-subscribed
        pk = wave_writelane(pk, uni(code | (off << 16)), L);
        if (c) maxl = L;
        code = (code + c) << 1; off += c;
    }
    if (maxl == 0u) return true;                                             // no code at all: a table of zeros (inflate_table accepts it for every kind)
    if (left > 0 && (codes || maxl != 1u)) return false;                     // incomplete
    if (lane >= 1 && lane <= 15) { canon[lane] = (u16)(pk & 0xFFFFu); canon[16 + lane] = (u16)cnt; canon[32 + lane] = (u16)(pk >> 16); }
    wave_sync();
    u32 nx = pk;                                                             // lane L: next code | next sorted index << 16 of length L
    for (u32 base = 0; base < nsym; base += ALZ_WAVE) {
        const u32 sym = base + (u32)lane, l = sym < nsym ? (u32)lens[sym] : 0u;
        const u32 mine = wave_bperm(l, nx);
        u32 rank = 0, add = 0;
#pragma unroll 1
        for (u32 L = 1; L <= maxl; L++) {
            const u64 m = wave_ballot(l == L);
            if (l == L) rank = mbcnt64(m);
            if ((u32)lane == L) add = (u32)__popcll(m);
        }
        nx += add * 0x10001u;
        if (l) {
            const u32 c = (mine & 0xFFFFu) + rank;
            sorted[(mine >> 16) + rank] = (u16)sym;
            const u32 r = __brev(c) >> (32u - l);
            if (l <= pb) { for (u32 k = r; k < tsize; k += 1u << l) tab[k] = (u16)((sym << 4) | l); }
            else tab[r & (tsize - 1u)] = (u16)INF_LONG;
        }
    }
    wave_sync();
    return true;
}

// the code at the low end of `x` (>= 15 stream bits, zero-padded): its entry (symbol << 4 | length), 0 when the set has no such code
__device__ __forceinline__ u32 inf_lookup(const u8* t, u32 tab_off, u32 pb, u32 canon_off, u32 sorted_off, u32 x) {
    u32 e = uni((u32)reinterpret_cast<const u16*>(t + tab_off)[x & ((1u << pb) - 1u)]);
    if ((e & 15u) == INF_LONG) {                                             // a code longer than the index: canonical compare, length by length
        const u16* canon = reinterpret_cast<const u16*>(t + canon_off);
        const u32 c15 = __brev(x) >> 17;                                     // the next 15 bits as an MSB-first number
        e = 0;
        for (u32 L = pb + 1u; L <= 15u; L++) {
            const u32 c = (c15 >> (15u - L)) - uni((u32)canon[L]);
            if (c < uni((u32)canon[16u + L])) {
                e = (uni((u32)reinterpret_cast<const u16*>(t + sorted_off)[uni((u32)canon[32u + L]) + c]) << 4) | L;
                break;
            }
        }
    }
    return e;
}

// HCLEN order of the code-length code's lengths (RFC 1951 3.2.7), 5 bits each
#define INF_ORDER_LO (16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55)
#define INF_ORDER_HI (12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30)

// the header of a dynamic block: HLIT, HDIST, HCLEN, the code-length code, the expanded lengths at INF_O_LENS.  false: s.eof or s.bad is set.
template <class SK>
__device__ __forceinline__ bool inf_dynamic_header(InCache& in, SK& sk, DecState& s, InfBits& b, u32 src_len, u8* t, int lane, u32& nlen, u32& ndist) {
    if (!inf_need(in, sk, s, b, src_len, 14u)) return false;
    nlen = inf_take(b, 5u) + 257u; ndist = inf_take(b, 5u) + 1u;
    const u32 ncl = inf_take(b, 4u) + 4u;
    if (nlen > 286u || ndist > 30u) { s.bad = true; return false; }
    u32 cl = 0;                                                              // lane k: the length of code-length symbol k
    for (u32 i = 0; i < ncl; i++) {
        if (!inf_need(in, sk, s, b, src_len, 3u)) return false;
        const u32 k = i < 12u ? (u32)(INF_ORDER_LO >> (5u * i)) & 31u : (u32)(INF_ORDER_HI >> (5u * (i - 12u))) & 31u;
        cl = wave_writelane(cl, uni(inf_take(b, 3u)), uni(k));
    }
    u8* const lens = t + INF_O_LENS;
    wave_sync();
    lens[lane] = (u8)cl;                                                     // (lanes 19..63 hold 0; the builder looks at 19 lengths)
    if (!inf_build(t, INF_O_LIT, INF_CL_PB, INF_O_LENS, 19u, INF_O_CDIST, INF_O_SDIST, true, lane)) { s.bad = true; return false; }
    const u32 total = nlen + ndist;
    u32 have = 0, prev = 0;
    while (have < total) {
        if (b.nb < 14u) inf_refill(in, sk, s, b, src_len);
        const u32 e = uni((u32)reinterpret_cast<const u16*>(t + INF_O_LIT)[(u32)b.bb & ((1u << INF_CL_PB) - 1u)]);
        const u32 l = e & 15u, sym = e >> 4;                                 // (a code-length code that has a code is complete, at most 7 bits long: l is 1..7)
        if (l == 0u) {                                                       // one with no code at all: zlib reads every length as a 1-bit 0, then misses symbol 256
            s.eof = (u64)b.nb + 8ull * (u64)(src_len - s.p) < (u64)(total - have);
            s.bad = !s.eof;
            return false;
        }
        if (l > b.nb) { s.eof = true; return false; }
        if (sym < 16u) {
            (void)inf_take(b, l);
            if (lane == 0) lens[have] = (u8)sym;
            have++; prev = sym;
        } else {
            const u32 eb = sym == 16u ? 2u : (sym == 17u ? 3u : 7u);
            if (l + eb > b.nb) { s.eof = true; return false; }
            (void)inf_take(b, l);
            const u32 rep = (sym == 18u ? 11u : 3u) + inf_take(b, eb);
            if (sym == 16u && have == 0u) { s.bad = true; return false; }    // nothing to repeat
            if (have + rep > total) { s.bad = true; return false; }          // the repeat runs past the last length
            if (sym != 16u) prev = 0;
            for (u32 j = (u32)lane; j < rep; j += ALZ_WAVE) lens[have + j] = (u8)prev;
            have += rep;
        }
    }
    wave_sync();
    if (uni((u32)lens[256]) == 0u) { s.bad = true; return false; }           // no end-of-block code
    return true;
}

// zlib's inflate over one raw DEFLATE stream.  `t`: ALZ_INFLATE_TABLES bytes of LDS.
template <class SK>
__device__ __forceinline__ void dec_inflate_serial(InCache& in, SK& sk, DecState& s, u32 src_len, u8* t, int lane) {
    InfBits b; b.bb = 0; b.nb = 0;
    bool fixed_ready = false;
    for (;;) {                                                               // one block per round
        if (!inf_need(in, sk, s, b, src_len, 3u)) return;
        const u32 hdr = inf_take(b, 3u), type = hdr >> 1;
        if (type == 3u) { s.bad = true; return; }
        if (type == 0u) {                                                    // stored
            (void)inf_take(b, b.nb & 7u);
            if (!inf_need(in, sk, s, b, src_len, 32u)) return;
            const u32 v = inf_take(b, 32u), len = v & 0xFFFFu;
            if ((len ^ 0xFFFFu) != (v >> 16)) { s.bad = true; return; }
            s.p -= b.nb >> 3; b.bb = 0; b.nb = 0;                            // whole bytes go back: the run is read at the input position
            const u32 have = src_len - s.p, n = len < have ? len : have;
            if (n) {
                if (!sk.run(in, s.p, (u64)n)) return;                        // (clipped: the sink sets ovf)
                s.p += n;
            }
            if (n < len) { s.eof = true; return; }
        } else {
            u32 nlen = 288u, ndist = 32u;
            if (type == 1u && !fixed_ready) {                                // the fixed lengths (RFC 1951 3.2.6); 32 distance codes of 5 bits
                u8* const lens = t + INF_O_LENS;
                wave_sync();
                for (u32 sym = (u32)lane; sym < 320u; sym += ALZ_WAVE)          // (five rounds of all lanes: 288 + 32 lengths)
                    lens[sym] = (u8)(sym < 144u ? 8u : (sym < 256u ? 9u : (sym < 280u ? 7u : (sym < 288u ? 8u : 5u))));
            }
            if (type == 2u && !inf_dynamic_header(in, sk, s, b, src_len, t, lane, nlen, ndist)) return;
            if (type == 2u || !fixed_ready) {
                if (!inf_build(t, INF_O_LIT, INF_LIT_PB, INF_O_LENS, nlen, INF_O_CLIT, INF_O_SLIT, false, lane)) { s.bad = true; return; }
                if (!inf_build(t, INF_O_DIST, INF_DIST_PB, INF_O_LENS + nlen, ndist, INF_O_CDIST, INF_O_SDIST, false, lane)) { s.bad = true; return; }
                fixed_ready = type == 1u;
            }
            for (;;) {                                                       // one symbol per round
                if (b.nb < 48u) inf_refill(in, sk, s, b, src_len);
                u32 e = inf_lookup(t, INF_O_LIT, INF_LIT_PB, INF_O_CLIT, INF_O_SLIT, (u32)b.bb);
                u32 used = e & 15u;
                const u32 sym = e >> 4;
                if (used == 0u) { s.eof = b.nb == 0u; s.bad = !s.eof; return; }   // a code the set does not have (zlib's invalid entry takes 1 bit)
                if (used > b.nb) { s.eof = true; return; }
                if (sym < 256u) {
                    (void)inf_take(b, used);
                    if (!sk.lit(sym)) return;
                    continue;
                }
                if (sym == 256u) { (void)inf_take(b, used); break; }
                if (sym > 285u) { s.bad = true; return; }                    // 286 / 287 of the fixed code
                u32 length, eb;
                if (sym < 265u) { length = sym - 254u; eb = 0; }
                else if (sym == 285u) { length = 258u; eb = 0; }
                else { eb = (sym - 261u) >> 2; length = 3u + ((4u + ((sym - 265u) & 3u)) << eb); }
                if (used + eb > b.nb) { s.eof = true; return; }
                length += (u32)(b.bb >> used) & ((1u << eb) - 1u);
                used += eb;
                e = inf_lookup(t, INF_O_DIST, INF_DIST_PB, INF_O_CDIST, INF_O_SDIST, (u32)(b.bb >> used));
                const u32 dl = e & 15u, dsym = e >> 4;
                if (dl == 0u) { s.eof = used >= b.nb; s.bad = !s.eof; return; }
                used += dl;
                if (used > b.nb) { s.eof = true; return; }
                if (dsym > 29u) { s.bad = true; return; }                    // 30 / 31 of the fixed code
                u32 dist, de;
                if (dsym < 4u) { dist = dsym + 1u; de = 0; }
                else { de = (dsym >> 1) - 1u; dist = 1u + ((2u + (dsym & 1u)) << de); }
                if (used + de > b.nb) { s.eof = true; return; }
                dist += (u32)(b.bb >> used) & ((1u << de) - 1u);
                used += de;                                                  // (<= 15 + 5 + 15 + 13 = 48)
                b.bb >>= used; b.nb -= used;
                if (dist > sk.produced()) { s.bad = true; return; }          // before the sink sees it: no zeros in front of the stream
                if (!sk.match(dist, (u64)length, ALZ_INFLATE_WINDOW)) return;
            }
        }
        if (hdr & 1u) { s.done = true; s.p -= b.nb >> 3; return; }           // BFINAL: src_used is just behind the byte of the last bit
    }
}

__device__ __forceinline__ int inf_status(const DecState& s) {
    if (s.eof) return ALZ_ST_INPUT_TRUNCATED;
    if (s.bad) return ALZ_ST_BAD_TOKEN;
    if (s.ovf) return ALZ_ST_OUTPUT_CAPACITY;
    return ALZ_ST_OK;                                                        // (s.done: the final end-of-block was read)
}
__device__ __forceinline__ void inf_write(alz_result* r, int lane, u32 dst_len, u32 src_used, int status, u32 src_len) {
    if (status == ALZ_ST_INPUT_TRUNCATED) src_used = src_len;
    if (lane == 0) { r->dst_len = dst_len; r->src_used = src_used; r->status = status; r->reserved = 0; }
}

// ------------------------------------------------------------------------------------------------ decode
// LDS per wavefront: ring | input cache | tables
__global__ __launch_bounds__(64) void alz_inflate_decode_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base,
                                                                const alz_stream* __restrict__ streams, const u32* __restrict__ index_list,
                                                                u32 count, alz_result* __restrict__ results) {
    constexpr u32 LW = ALZ_INFLATE_LW;
    static_assert(LW >= 1024u && (LW & (LW - 1u)) == 0u, "the ring is a power of two");
    __shared__ __attribute__((aligned(16))) u8 lds[LW + ALZ_INFLATE_CACHE + ALZ_INFLATE_TABLES];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    typedef OutWin<true> OW;
    OW out; out.init(dst_base + st.dst_off, cap, lds, LW, lane);
    InCache in; in.init(src_base + st.src_off, src_len, lds + LW, lane, ALZ_INFLATE_QCH);
    DecState s; dec_state_init(s);
    DirectSink<OW> sk(out, s);
    dec_inflate_serial(in, sk, s, src_len, lds + LW + ALZ_INFLATE_CACHE, lane);
    out.finish();
    inf_write(&results[sid], lane, out.produced, s.p, inf_status(s), src_len);
}

// ------------------------------------------------------------------------------------------------ measure
// The counting sink: dst_cap only bounds the count (a clipped symbol reports dst_len = dst_cap, as the decoder does).
struct InfCountSink {
    DecState& s; u32 n, cap;
    __device__ __forceinline__ InfCountSink(DecState& st, u32 c) : s(st), n(0), cap(c) {}
    __device__ __forceinline__ u32 produced() const { return n; }
    __device__ __forceinline__ void ensure(InCache& in, u32 p, u32 need) { in.ensure(p, need); }
    __device__ __forceinline__ bool add(u64 len) {
        if (len > (u64)(cap - n)) { s.ovf = true; n = cap; return false; }
        n += (u32)len;
        return true;
    }
    __device__ __forceinline__ bool lit(u32) { return add(1u); }
    __device__ __forceinline__ bool match(u32, u64 len, u32) { return add(len); }
    __device__ __forceinline__ bool run(InCache&, u32, u64 len) { return add(len); }
};

__global__ __launch_bounds__(64) void alz_inflate_measure_kernel(const u8* __restrict__ src_base, const alz_stream* __restrict__ streams,
                                                                 const u32* __restrict__ index_list, u32 count, alz_result* __restrict__ results) {
    __shared__ __attribute__((aligned(16))) u8 lds[ALZ_INFLATE_CACHE + ALZ_INFLATE_TABLES];
    const u32 bid = blockIdx.x;
    if (bid >= count) return;
    const int lane = (int)threadIdx.x;
    const u32 sid = index_list ? index_list[bid] : bid;
    const alz_stream st = streams[sid];
    const u32 src_len = uni(st.src_len), cap = uni(st.dst_cap);
    InCache in; in.init(src_base + st.src_off, src_len, lds, lane, ALZ_INFLATE_QCH);
    DecState s; dec_state_init(s);
    InfCountSink sk(s, cap);
    dec_inflate_serial(in, sk, s, src_len, lds + ALZ_INFLATE_CACHE, lane);
    inf_write(&results[sid], lane, sk.n, s.p, inf_status(s), src_len);
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t alz_launch_inflate_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* streams, const u32* index,
                                     u32 count, alz_result* results) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_inflate_decode_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, streams, index, count, results);
    return hipGetLastError();
}

hipError_t alz_launch_inflate_measure(hipStream_t stream, const void* d_src, const alz_stream* streams, const u32* index, u32 count, alz_result* results) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_inflate_measure_kernel, dim3(count), dim3(64), 0, stream, (const u8*)d_src, streams, index, count, results);
    return hipGetLastError();
}

// ================================================================================================ the encoder (alz_deflate_*)
// alz_inflate.h describes the launches and holds the code builder (host and device code, tested on the CPU).  Grid mapping: one wavefront
// (= one 64-thread workgroup) per BLOCK of ALZ_DEFLATE_BLOCK input bytes, so one long stream fills the GPU as a batch of short ones does.
//
// find.  The history of a DEFLATE encoder is its input: a block first inserts the 32 KiB in front of it, then itself, 64 positions per
// step.  LDS holds head[2^14] (the newest position + 1 per hash of three bytes) and prev[32 Ki] (per position mod 32 Ki the distance to the
// one before it on its chain; 0 ends it).  A step reads the heads, links its 64 positions -- to the nearest EARLIER LANE with the same
// three bytes if there is one (63 shuffles), else to the head -- and only then publishes them (atomicMax: the newest wins whatever the
// order).  So the chains, and with them the tokens, are a function of the stream's bytes and the level alone.  Inside the block every lane
// then walks its chain (level: how many candidates, which length ends the walk), and a wave-uniform loop picks the tokens greedily or, from
// level 4 on, lazily: a position whose successor has a longer match becomes a literal.  A slot of prev that a position 32 KiB later has
// overwritten can lead the walk to a position that is no real candidate; every candidate is compared byte by byte, and the walk ends at
// distance 32 768 and at the stream's start, so such a slot costs a compare.  Matches never leave the block, never exceed 258 bytes.
// emit.  Each lane turns a token into at most 48 bits, a wave prefix sum places them, and the lanes OR them into a zeroed image of the
// whole block in LDS (a block is never larger than its stored form: 32 709 bytes); the image is then stored at the block's byte offset.
#define DFL_HASH_BITS 14u
#define DFL_WIN 32768u
#define DFL_STAGE_WORDS ((ALZ_DEFLATE_BLOCK + 64u) / 4u)

__device__ __forceinline__ u32 dfl_ld4(const u8* p) { u32 v; __builtin_memcpy(&v, p, 4); return v; }
// equal bytes at a and b, at most `maxlen` (both readable that far)
__device__ __forceinline__ u32 dfl_match_len(const u8* a, const u8* b, u32 maxlen) {
    u32 i = 0;
    while (i + 4u <= maxlen) {
        const u32 x = dfl_ld4(a + i) ^ dfl_ld4(b + i);
        if (x) return i + ((u32)__builtin_ctz(x) >> 3);
        i += 4u;
    }
    while (i < maxlen && a[i] == b[i]) i++;
    return i;
}

__global__ __launch_bounds__(64) void alz_deflate_find_kernel(const u8* __restrict__ src_base, const alz_stream* __restrict__ streams,
                                                              const alz_deflate_blk* __restrict__ blocks, u32 nblocks, int level, u32 flags,
                                                              u32* __restrict__ tokens, alz_deflate_plan* __restrict__ plans) {
    __shared__ u32 head[1u << DFL_HASH_BITS];
    __shared__ unsigned short prev[DFL_WIN];
    __shared__ u32 lit_freq[ALZ_DEFLATE_NLIT + 2], dist_freq[ALZ_DEFLATE_NDIST + 2];
    __shared__ alz_deflate_work work;
    __shared__ __attribute__((aligned(16))) alz_deflate_plan plan;
    __shared__ u32 sizes[3];
    const u32 bid = blockIdx.x;
    if (bid >= nblocks) return;
    const u32 lane = threadIdx.x;
    const alz_deflate_blk blk = blocks[bid];
    const alz_stream st = streams[blk.sid];
    const u8* src = src_base + st.src_off;
    const u32 n = uni(st.src_len);
    const u32 bs = uni(blk.k) * ALZ_DEFLATE_BLOCK;
    const u32 blen = n - bs < ALZ_DEFLATE_BLOCK ? n - bs : ALZ_DEFLATE_BLOCK;
    const u32 bend = bs + blen;
    const bool final = bend == n;
    u32* tok = tokens + blk.tok_at;

    for (u32 i = lane; i < sizeof(plan) / 4u; i += 64u) ((u32*)&plan)[i] = 0;
    for (u32 i = lane; i < ALZ_DEFLATE_NLIT + 2; i += 64u) lit_freq[i] = 0;
    if (lane < ALZ_DEFLATE_NDIST + 2) dist_freq[lane] = 0;
    u32 ntok = 0;
    if (level > 0 && blen > 0) {
        for (u32 i = lane; i < (1u << DFL_HASH_BITS); i += 64u) head[i] = 0;
        for (u32 i = lane; i < DFL_WIN; i += 64u) prev[i] = 0;
        __syncthreads();
        const u32 chain_max = alz_deflate_level_chain(level), nice = alz_deflate_level_nice(level);
        const bool lazy = alz_deflate_level_lazy(level);
        u32 skip = 0;                                        // positions of the coming steps that the last match covers
        for (u32 gs = bs > DFL_WIN ? bs - DFL_WIN : 0u; gs < bend; gs += 64u) {
            const u32 p = gs + lane;
            const bool hashable = p + 3u <= n;
            u32 tri = 0xFFFFFFFFu, h = 0;
            if (hashable) {
                tri = (u32)src[p] | ((u32)src[p + 1] << 8) | ((u32)src[p + 2] << 16);
                h = (tri * 0x9E3779B1u) >> (32u - DFL_HASH_BITS);
            }
            const u32 old = hashable ? head[h] : 0u;
            u32 delta = 0;
#pragma unroll 1
            for (u32 d = 1; d < 64u; d++) {
                const u32 t = __shfl_up(tri, d);
                if (lane >= d && t == tri && !delta) delta = d;
            }
            if (!hashable) delta = 0;
            else if (!delta && old) delta = p + 1u - old;
            if (delta > DFL_WIN) delta = 0;
            if (hashable) prev[p & (DFL_WIN - 1u)] = (unsigned short)delta;
            __syncthreads();
            if (hashable) atomicMax(&head[h], p + 1u);
            __syncthreads();
            if (gs < bs) continue;                            // the window in front of the block: inserted only
            // ---- the best match of every position
            const u32 maxlen = p < bend ? (bend - p < 258u ? bend - p : 258u) : 0u;
            u32 best = 0, best_dist = 0;
            if (maxlen >= 3u && hashable) {
                u32 cur = p, dl = delta;
                for (u32 c = chain_max; dl && c; c--) {
                    if (dl > cur) break;
                    cur -= dl;
                    const u32 dist = p - cur;
                    if (dist > DFL_WIN) break;
                    if (best < 3u || src[cur + best] == src[p + best]) {
                        const u32 len = dfl_match_len(src + cur, src + p, maxlen);
                        if (len > best) { best = len; best_dist = dist; }
                        if (best >= nice || best >= maxlen) break;
                    }
                    dl = prev[cur & (DFL_WIN - 1u)];
                }
                if (best < 3u || (best == 3u && best_dist > 4096u)) best = 0;
            }
            // ---- the parse of these 64 positions: wave-uniform
            const u32 nvalid = bend - gs < 64u ? bend - gs : 64u;
            u64 tmask = 0, lmask = 0;
            u32 cur = skip;
            while (cur < nvalid) {
                u32 L = (u32)__builtin_amdgcn_readlane((int)best, (int)cur);
                if (lazy && L >= 3u && cur + 1u < nvalid && (u32)__builtin_amdgcn_readlane((int)best, (int)(cur + 1u)) > L) L = 0;
                tmask |= 1ull << cur;
                if (L < 3u) { lmask |= 1ull << cur; cur += 1u; } else cur += L;
            }
            skip = cur - nvalid;
            if ((tmask >> lane) & 1ull) {
                const u32 at = ntok + (u32)__popcll(tmask & ((1ull << lane) - 1ull));
                if ((lmask >> lane) & 1ull) {
                    const u32 b = src[p];
                    tok[at] = b;
                    atomicAdd(&lit_freq[b], 1u);
                } else {
                    u32 eb, ev;
                    tok[at] = 0x80000000u | ((best - 3u) << 16) | (best_dist - 1u);
                    atomicAdd(&lit_freq[alz_deflate_len_sym(best, &eb, &ev)], 1u);
                    atomicAdd(&dist_freq[alz_deflate_dist_sym(best_dist, &eb, &ev)], 1u);
                }
            }
            ntok += (u32)__popcll(tmask);
        }
    }
    __syncthreads();
    if (lane == 0) {
        lit_freq[256] = 1;
        alz_deflate_plan_block(lit_freq, dist_freq, blen, ntok, final, level == 0, (flags & 1u) != 0, &work, &plan, sizes);
    }
    __syncthreads();
    for (u32 i = lane; i < sizeof(plan) / 4u; i += 64u) ((u32*)&plans[bid])[i] = ((const u32*)&plan)[i];
}

// one lane per stream: where its blocks go, whether they fit, the result
__global__ __launch_bounds__(64) void alz_deflate_place_kernel(const alz_stream* __restrict__ streams, u32 n, const u32* __restrict__ first,
                                                               alz_deflate_plan* __restrict__ plans, alz_result* __restrict__ results) {
    const u32 sid = blockIdx.x * 64u + threadIdx.x;
    if (sid >= n) return;
    u64 at = 0;
    for (u32 b = first[sid]; b < first[sid + 1]; b++) { plans[b].dst_at = (u32)at; at += plans[b].bytes; }
    const bool fits = at <= (u64)streams[sid].dst_cap;
    alz_result r;
    r.dst_len = fits ? (u32)at : 0u; r.src_used = fits ? streams[sid].src_len : 0u; r.status = fits ? ALZ_ST_OK : ALZ_ST_OUTPUT_CAPACITY; r.reserved = 0;
    results[sid] = r;
}

// `nb` bits of `v` (at most 48) at bit `pos` of the zeroed image
__device__ __forceinline__ void dfl_put(u32* stage, u32 pos, u64 v, u32 nb) {
    if (!nb) return;
    const u32 w = pos >> 5, sh = pos & 31u;
    const u32 a0 = (u32)(v << sh);
    const u64 rest = sh ? v >> (32u - sh) : v >> 32;
    if (a0) atomicOr(&stage[w], a0);
    if ((u32)rest) atomicOr(&stage[w + 1], (u32)rest);
    if ((u32)(rest >> 32)) atomicOr(&stage[w + 2], (u32)(rest >> 32));
}

__global__ __launch_bounds__(64) void alz_deflate_emit_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                              const alz_deflate_blk* __restrict__ blocks, u32 nblocks, const u32* __restrict__ tokens,
                                                              const alz_deflate_plan* __restrict__ plans, const alz_result* __restrict__ results) {
    __shared__ u32 stage[DFL_STAGE_WORDS];
    __shared__ unsigned short lit_code[288], dist_code[32], blc[16];
    __shared__ u8 lit_len[288], dist_len[32];
    const u32 bid = blockIdx.x;
    if (bid >= nblocks) return;
    const u32 lane = threadIdx.x;
    const alz_deflate_blk blk = blocks[bid];
    if (results[blk.sid].status != ALZ_ST_OK) return;        // the stream does not fit: nothing of it is written
    const alz_stream st = streams[blk.sid];
    const alz_deflate_plan* pl = &plans[bid];
    const u32 n = uni(st.src_len), bs = uni(blk.k) * ALZ_DEFLATE_BLOCK;
    const u32 blen = n - bs < ALZ_DEFLATE_BLOCK ? n - bs : ALZ_DEFLATE_BLOCK;
    const bool final = bs + blen == n;
    const u32 type = uni(pl->type), bytes = uni(pl->bytes), ntok = uni(pl->ntok);
    u8* dst = dst_base + st.dst_off + pl->dst_at;
    if (type == ALZ_DEFLATE_STORED) {
        if (lane < 5u) dst[lane] = lane == 0 ? (u8)final : (u8)(((lane < 3u ? blen : ~blen) >> (8u * ((lane - 1u) & 1u))) & 0xFFu);
        const u8* s = src_base + st.src_off + bs;
        for (u32 i = lane; i < blen; i += 64u) dst[5u + i] = s[i];
        return;
    }
    for (u32 i = lane; i < DFL_STAGE_WORDS; i += 64u) stage[i] = 0;
    for (u32 i = lane; i < 288u; i += 64u) lit_len[i] = type == ALZ_DEFLATE_DYNAMIC ? pl->lit_len[i] : (u8)alz_deflate_fixed_len(i);
    if (lane < 32u) dist_len[lane] = type == ALZ_DEFLATE_DYNAMIC ? pl->dist_len[lane] : (u8)5;
    __syncthreads();
    if (lane == 0) alz_deflate_codes(lit_len, 288u, lit_code, blc);
    __syncthreads();
    if (lane == 0) alz_deflate_codes(dist_len, 32u, dist_code, blc);
    __syncthreads();
    u32 pos = 3u;
    if (lane == 0) dfl_put(stage, 0, (u64)((final ? 1u : 0u) | (type << 1)), 3u);
    if (type == ALZ_DEFLATE_DYNAMIC) {
        const u32 hb = uni(pl->hdr_bits);
        for (u32 i = lane; i * 8u < hb; i += 64u) dfl_put(stage, 3u + i * 8u, (u64)pl->hdr[i], 8u);   // (the bits of the last byte behind hdr_bits are zero)
        pos += hb;
    }
    const u32* tok = tokens + blk.tok_at;
    for (u32 base = 0; base <= ntok; base += 64u) {
        const u32 i = base + lane;
        u64 v = 0; u32 nb = 0;
        if (i < ntok) {
            const u32 t = tok[i];
            if (!(t & 0x80000000u)) { v = lit_code[t]; nb = lit_len[t]; }
            else {
                u32 eb, ev;
                const u32 ls = alz_deflate_len_sym(((t >> 16) & 0xFFu) + 3u, &eb, &ev);
                v = lit_code[ls]; nb = lit_len[ls];
                v |= (u64)ev << nb; nb += eb;
                const u32 ds = alz_deflate_dist_sym((t & 0x7FFFu) + 1u, &eb, &ev);
                v |= (u64)dist_code[ds] << nb; nb += dist_len[ds];
                v |= (u64)ev << nb; nb += eb;
            }
        } else if (i == ntok) { v = lit_code[256]; nb = lit_len[256]; }
        u32 incl = nb;
#pragma unroll
        for (u32 d = 1; d < 64u; d <<= 1) { const u32 t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        if (pos + incl <= 8u * bytes) dfl_put(stage, pos + incl - nb, v, nb);   // (always: the plan counted these very bits)
        pos += (u32)__builtin_amdgcn_readlane((int)incl, 63);
    }
    // the joining: three zero bits and the padding are already there
    if (!final && lane == 0) dfl_put(stage, 8u * (bytes - 2u), 0xFFFFull, 16u);
    __syncthreads();
    for (u32 i = lane; i < bytes; i += 64u) dst[i] = (u8)(stage[i >> 2] >> (8u * (i & 3u)));
}

hipError_t alz_launch_deflate_encode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams, u32 n,
                                     const alz_deflate_blk* d_blocks, u32 nblocks, const u32* d_first, u32* d_tokens,
                                     alz_deflate_plan* d_plans, int level, u32 flags, alz_result* d_results) {
    if (n == 0 || nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_deflate_find_kernel, dim3(nblocks), dim3(64), 0, stream, (const u8*)d_src, d_streams, d_blocks, nblocks, level, flags, d_tokens, d_plans);
    hipLaunchKernelGGL(alz_deflate_place_kernel, dim3((n + 63u) / 64u), dim3(64), 0, stream, d_streams, n, d_first, d_plans, d_results);
    hipLaunchKernelGGL(alz_deflate_emit_kernel, dim3(nblocks), dim3(64), 0, stream, (const u8*)d_src, (u8*)d_dst, d_streams, d_blocks, nblocks,
                       (const u32*)d_tokens, (const alz_deflate_plan*)d_plans, (const alz_result*)d_results);
    return hipGetLastError();
}
