// alz_encode_bits.h -- the three bit-stream LZ bodies of the encoder, included by alz_encode.hip: CRILAYLA.CompressHeaderless (CRI/CRILAYLA.cs:190-258),
// ALLZ.CompressHeaderless (Specialized/ALLZ.cs:129-174) and aPLib.CompressHeaderless (Formats/Common/aPLib.cs:183-286).  All three run LzChainMatchFinder,
// so kernels A and B, the roles walk and the capped-cursor search are those of alz_encode.hip; what stands here is their emission from the walk's start
// mask, twice per format, and the kernel that hands the finder CRILAYLA's reversed source.  (Internal formats behind the public enum: ALZ_ENCFMT_*, alz_bitlz.h.)
//   one lane per stream      cri_emit_lone, allz_emit_lone, aplib_emit_lone: three bodies of enc_emit_kernel, the exact mode's -- the managed loops token by
//                            token, the device's independent restatement every GPU test holds the default mode against: they share nothing with it
//   one wavefront per stream enc_bits_cri_kernel, enc_bits_allz_kernel, enc_gamma_ap_kernel, the default: one lane per position of a 64-position window, placement
//                            by prefix sums.  Each is its grammar (cri_token, allz_field, ap_token) around ONE windowed emitter: StreamView, window_starts, BitWindow, SidePlacer

__device__ __forceinline__ void write_result(alz_result* results, u32 sid, u32 dst_len, u32 src_len, int status) {
    alz_result r; r.dst_len = dst_len; r.src_used = src_len; r.status = status; r.reserved = 0; results[sid] = r;
}
// the serial emitters' finder over a whole stream of n bytes
__device__ __forceinline__ Finder finder_over(const mentry* m, const u64* mask, int n) { Finder f; f.m = m; f.position = 0; f.n = n; f.limit = n - 4; f.mask = mask; return f; }

// ---------------------------------------------------------------------------------------------- the windowed emitter
// A wavefront walks its stream in windows of 64 positions, one lane per position.  Per window: window_starts says which lanes start a match and where
// the match before each lane ends; the format's grammar turns that into a token of some bits per lane; scan_add of the widths gives every lane its
// bit offset and the lanes OR their fields into a bit string in LDS (ds_or on dwords: a lane places its field without knowing whose bits share its
// bytes; through shuffles that would be a segmented OR-scan over fields of unequal width); the window's whole bytes are stored side by side, and the
// byte the window ends in travels to the next one in a register.  Formats that put other bytes between their flag bytes (ALLZ's runs, aPLib's
// payload) place both with a SidePlacer.

// one stream of a launch: where its source, its output, its match array and its start mask lie
struct StreamView {
    u32 sid, src_len, cap, aux0; int n, nwords;                         // nwords: the mask words the roles walk may have written
    const u8* src; u8* dst; const mentry* m; const u64* mask;
    __device__ __forceinline__ StreamView(const u8* src_base, u8* dst_base, const alz_stream* streams, const u32* index_list, const u64* pos_off,
                                          const mentry* match, const u64* startmask, u32 i) {
        sid = index_list[i]; const alz_stream st = streams[sid];
        src_len = st.src_len; cap = st.dst_cap; aux0 = st.aux0; n = (int)st.src_len;
        src = src_base + st.src_off; dst = dst_base + st.dst_off;
        m = match + pos_off[sid]; mask = startmask + (pos_off[sid] >> 6);
        nwords = n >= 4 ? ((n - 4) >> 6) + 1 : 0;
    }
    __device__ __forceinline__ u64 mask_word(int P) const { return (P >> 6) < nwords ? mask[P >> 6] : 0ull; }
};

// The window at P, whose mask word is mw: whether this lane's position starts a match, the match (the array's distance field as it stands, the length
// exact: the roles walk has recomputed what kernel B had capped), and `prev`: where the last match that starts in front of this lane ends -- the
// exclusive prefix maximum of the match ends, at least `cover`, the end the windows before have left.  Advances `cover` over this window.
struct WinStarts { bool start; u32 D, L, prev; };
__device__ __forceinline__ WinStarts window_starts(const StreamView& s, int P, u64 mw, u32& cover) {
    const int lane = (int)threadIdx.x, p = P + lane;
    WinStarts w = { (bool)((mw >> lane) & 1ull), 0u, 0u, 0u };
    if (w.start) { uint2 r = m_unpack(s.m[p]); if (r.y == ALZ_M_LONG) r.y = s.m[p + 1]; w.D = r.x; w.L = r.y; }
    const u32 incl = scan_max(w.start ? (u32)p + w.L : 0u);
    w.prev = (u32)__builtin_amdgcn_update_dpp(0, (int)incl, 0x138, 0xF, 0xF, false);          // wave_shr:1 -> the ends of the matches that start in the lanes below
    if (w.prev < cover) w.prev = cover;
    const u32 last = (u32)__builtin_amdgcn_readlane((int)incl, 63); if (last > cover) cover = last;
    return w;
}

// The bit string of one window in DWORDS dwords of LDS and the stream's running state.  MSB: a byte fills from its top bit (CRILAYLA's SetBits,
// FlagWriter(Endian.Big)), so bit t is bit 31 - t % 32 of dword t / 32; otherwise from its lowest (FlagWriter(Endian.Little)): bit t % 32.
// A window: open(), offset() of this lane's width, sync(), put()s, seal(), the stores of byte_at(j) for j < nfull, close().
template <bool MSB, int DWORDS>
struct BitWindow {
    u32* buf;                                                           // LDS
    u64 G = 0; u32 carry = 0;                                           // bits placed so far; the bits of the byte they end in (MSB: its top G % 8, else its low ones)
    u32 phase = 0, bits = 0, end = 0, nfull = 0;                        // of the open window: G % 8, the bits of its tokens, phase + bits, its whole bytes
    __device__ __forceinline__ void sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
    // an empty string behind the carried byte; the bit of it this lane's `width` bits begin at
    __device__ __forceinline__ void open() { for (int j = (int)threadIdx.x; j < DWORDS; j += 64) buf[j] = j == 0 ? (MSB ? carry << 24 : carry) : 0u; phase = (u32)G & 7u; }
    __device__ __forceinline__ u32 offset(u32 width) { const u32 incl = scan_add(width); bits = (u32)__builtin_amdgcn_readlane((int)incl, 63); return phase + incl - width; }
    __device__ __forceinline__ void put(u32 t, u32 v, u32 nb) {         // nb <= 32 bits of v at bit t, most significant first
        static_assert(MSB); const u64 x = (u64)v << (64u - (t & 31u) - nb);
        atomicOr(&buf[t >> 5], (u32)(x >> 32));
        if ((u32)x) atomicOr(&buf[(t >> 5) + 1u], (u32)x);
    }
    __device__ __forceinline__ void put(u32 t, u64 v) {                 // v < 2^61 at bit t, least significant first
        static_assert(!MSB); const u32 s = t & 31u, d = t >> 5;
        const u64 lo = v << s;
        if ((u32)lo) atomicOr(&buf[d], (u32)lo);
        if ((u32)(lo >> 32)) atomicOr(&buf[d + 1u], (u32)(lo >> 32));
        if (s && (u32)(v >> (64u - s))) atomicOr(&buf[d + 2u], (u32)(v >> (64u - s)));
    }
    __device__ __forceinline__ void fill_ones(int l, u32 at, u32 len) { // lane l's `len` one-bits from its bit `at` by the whole wavefront: partial dword, full dwords, partial dword
        const u32 o0 = (u32)__builtin_amdgcn_readlane((int)at, l), o1 = o0 + (u32)__builtin_amdgcn_readlane((int)len, l);
        for (u32 j = (o0 >> 5) + threadIdx.x; j <= ((o1 - 1u) >> 5); j += 64u) {
            const u32 lo = o0 > 32u * j ? o0 - 32u * j : 0u, hi = o1 < 32u * j + 32u ? o1 - 32u * j : 32u;
            atomicOr(&buf[j], (0xFFFFFFFFu >> lo) & (hi < 32u ? ~(0xFFFFFFFFu >> hi) : 0xFFFFFFFFu));
        }
    }
    __device__ __forceinline__ u32 byte_at(u32 j) const { return (buf[j >> 2] >> (MSB ? 24u - 8u * (j & 3u) : 8u * (j & 3u))) & 0xFFu; }
    __device__ __forceinline__ u32 seal() { sync(); end = phase + bits; return nfull = end >> 3; }          // every field is in: the string's whole bytes are [0, nfull)
    __device__ __forceinline__ void close() { carry = (end & 7u) ? byte_at(nfull) : 0u; G += (u64)bits; sync(); }   // they are stored: the partial one travels on
};

// Side bytes between the flag bytes (ALLZ's literal runs, aPLib's payload bytes), as FlagWriter orders them.  A lane hands `cnt` side bytes over behind
// F flag bytes of the window -- F = ceil(B / 8) with B the window's bits written by then: FlushIfNecessary lets them out at once when B % 8 == 0,
// otherwise they wait for the open flag byte -- so they land at base + byte0 + F + the side bytes before them, and flag byte j of the window stands at
// base + byte0 + j + the side bytes handed over with F <= j.  F is monotone over the lanes, so a binary search over the window's prefix maxima of F
// counts those; the side bytes of earlier windows all have F <= the first NEW flag byte of this one, and the byte carried in was placed by the window
// it began in (carry_pos).  base: what stands in front of the first flag byte (aPLib's raw source[0]).
struct SidePlacer {
    u32* key; u32* rsum;                                                // LDS, per lane: the largest F so far in the window, the side bytes handed over so far
    u32 base, rtot = 0, carry_pos = 0;                                  // side bytes of the windows before; the place of the flag byte the bits end in
    u32 byte0 = 0, rincl = 0;                                           // of the open window: the flag byte its string starts with, this lane's inclusive side-byte count
    // between the window's open() and sync(): this lane hands over cnt bytes behind F flag bytes (F counts when cnt != 0 only); returns where they go
    template <class W> __device__ __forceinline__ u32 open(const W& w, u32 cnt, u32 F) {
        rincl = scan_add(cnt); key[threadIdx.x] = scan_max(cnt ? F : 0u); rsum[threadIdx.x] = rincl;
        byte0 = (u32)(w.G >> 3);
        return base + byte0 + F + rtot + rincl - cnt;
    }
    __device__ __forceinline__ u32 where(u32 phase, u32 j) const { return (j == 0u && phase) ? carry_pos : place(j); }   // (the byte carried in keeps its place)
    __device__ __forceinline__ u32 place(u32 j) const {
        u32 lo = 0, hi = 64;                                            // lanes [0, lo) have key <= j
        while (lo < hi) { const u32 mid = (lo + hi) >> 1; if (key[mid] <= j) lo = mid + 1u; else hi = mid; }
        return base + byte0 + j + rtot + (lo ? rsum[lo - 1u] : 0u);
    }
};
// the end of a window with side bytes: its whole flag bytes through store(at, byte), the partial one on with the place it was given
template <class W, class Store> __device__ __forceinline__ void close_placed(W& w, SidePlacer& pl, Store store) {
    const u32 nfull = w.seal();
    for (u32 j = threadIdx.x; j < nfull; j += 64u) store(pl.where(w.phase, j), w.byte_at(j));
    if (w.end & 7u) pl.carry_pos = pl.where(w.phase, nfull);
    pl.rtot += (u32)__builtin_amdgcn_readlane((int)pl.rincl, 63);
    w.close();
}

// ---------------------------------------------------------------------------------------------- CRILAYLA written
// (a stream's descriptor counts its source from src_base, wherever it lies: rev_delta = rev_base - src_base takes the offset back into the scratch)
__global__ __launch_bounds__(256) void enc_bits_reverse_kernel(const u8* __restrict__ src_base, u8* __restrict__ rev_base, u64 rev_delta,
                                                               const alz_stream* __restrict__ streams, const u64* __restrict__ orig_off,
                                                               const u32* __restrict__ index_list) {
    const u32 sid = index_list[blockIdx.y];
    const u32 n = streams[sid].src_len;
    const u8* s = src_base + orig_off[sid];
    u8* d = rev_base + (streams[sid].src_off - rev_delta);
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) d[i] = s[n - 1u - i];
}

// bits of a CRILAYLA match's length code: fields of 2, 3, 5, 8, 8, ... bits, an all-ones field meaning "more"  CRILAYLA.cs:228-238
__device__ __forceinline__ u32 cri_len_bits(u32 length) {
    const u32 rem = length - 3u;
    return rem < 3u ? 2u : rem < 10u ? 5u : rem < 41u ? 10u : 10u + 8u * ((rem - 41u) / 255u + 1u);
}

// SetBits  CRILAYLA.cs:260-279 with the body's place known beforehand: the managed code fills its array from the last byte downwards, most
// significant bit first, and hands over the top `total` bytes -- so forward bit b is bit 7 - b % 8 of byte total - 1 - b / 8 of the body.
struct CriBits {
    u8* p; u32 at, total; u64 acc; u32 n;                                  // at: index of the byte the next eight bits fill (below `total`: the sizing walk's count)
    __device__ __forceinline__ void put(u32 v, u32 bits) {               // bits <= 14
        acc = (acc << bits) | v; n += bits;
        while (n >= 8u) { n -= 8u; if (at < total) p[at] = (u8)(acc >> n); at--; }
    }
    __device__ __forceinline__ void end() { if (n && at < total) p[at] = (u8)(acc << (8u - n)); }   // if (bitsLeft != 8) destination[dst--] = bitBuffer  :243-244
};

// CRILAYLA.CompressHeaderless  :208-246 over the REVERSED source (the stream's descriptor points at it).  Two walks over the start mask: the
// first adds up the bits, the second writes them -- the body occupies [0, ceil(bits / 8)) of the stream's output.  false: no room (nothing written)
__device__ bool cri_emit_lone(const u8* src, int n, const mentry* m, const u64* mask, u8* dst, u32 cap, u32& len_out) {
    Finder mf = finder_over(m, mask, n);
    u64 bits = 0; int sp = 0;
    for (;;) {
        const Match mt = mf.next();
        bits += 9ull * (u64)(mt.offset - sp);
        if (mt.length == 0) break;
        bits += 14ull + cri_len_bits((u32)mt.length);
        sp = mt.offset + mt.length;
    }
    const u64 total = (bits + 7ull) >> 3;
    len_out = (u32)total;
    if (total > (u64)cap) return false;
    if (total == 0ull) return true;
    Finder mw = finder_over(m, mask, n);
    CriBits w = { dst, (u32)total - 1u, (u32)total, 0ull, 0u };
    sp = 0;
    for (;;) {
        const Match mt = mw.next();
        for (int plain = mt.offset - sp; plain != 0; plain--) w.put(src[sp++], 9u);         // the literal's 0-bit and its byte  :217-218
        if (mt.length == 0) break;
        w.put(0x2000u | (u32)(mt.distance - 3), 14u);                                       // is match, distance - 3 in 13 bits  :225-226
        u32 rem = (u32)mt.length - 3u;
        if (rem < 3u) w.put(rem, 2u);
        else {
            w.put(3u, 2u); rem -= 3u;
            if (rem < 7u) w.put(rem, 3u);
            else {
                w.put(7u, 3u); rem -= 7u;
                if (rem < 31u) w.put(rem, 5u);
                else {
                    w.put(31u, 5u); rem -= 31u;
                    while (rem >= 255u) { w.put(255u, 8u); rem -= 255u; }
                    w.put(rem, 8u);
                }
            }
        }
        sp += mt.length;
    }
    w.end();
    return true;
}

// ---- CRILAYLA by the whole wavefront.  A position is a literal (9 bits), the start of a match (14 bits, then the length code) or covered by a
// match (nothing).  A first walk over the windows adds up the bits -- the body has T = ceil(bits / 8) bytes, nothing is written unless it fits, and
// forward bit b is bit 7 - b % 8 of byte T - 1 - b / 8: the window's byte k goes to dst[T - 1 - k], no side bytes --, the second places them; the
// long run of one-bits of a length code (up to 257 fields of eight) is filled in by the whole wavefront.
// The bit string of a window: at most 64 tokens of 24 bits, two of them (a match of 44 bytes and more covers 44 positions) with up to
// 8 * 257 + 8 bits more, 7 bits of the byte carried in: 5 719 bits, 179 dwords and one for a field's low half.
#define ALZ_CRI_WIN_DWORDS 192
struct CriTok { u32 width, hv, hb, ones, tail; };                       // hb bits of hv, then `ones` one-bits and the 8 bits of `tail` (ones != 0 only)
__device__ __forceinline__ CriTok cri_token(bool start, bool lit, u32 byte, u32 D, u32 L) {
    CriTok t = { 0u, 0u, 0u, 0u, 0u };
    if (lit) { t.hv = byte; t.hb = 9u; t.width = 9u; }                  // the literal's 0-bit and its byte  :217-218
    else if (start) {
        const u32 head = 0x2000u | (D - 3u), rem = L - 3u;              // is match, distance - 3 in 13 bits  :225-226, the length code  :228-238
        if (rem < 3u) { t.hv = (head << 2) | rem; t.hb = 16u; }
        else if (rem < 10u) { t.hv = (head << 5) | 0x18u | (rem - 3u); t.hb = 19u; }
        else if (rem < 41u) { t.hv = (head << 10) | 0x3E0u | (rem - 10u); t.hb = 24u; }
        else { t.hv = (head << 10) | 0x3FFu; t.hb = 24u; t.ones = 8u * ((rem - 41u) / 255u); t.tail = (rem - 41u) % 255u; }
        t.width = t.hb + (rem >= 41u ? t.ones + 8u : 0u);
    }
    return t;
}
// the token of this lane's position in the window at P (the sizing walk wants the widths only: no literal is loaded for it)
__device__ __forceinline__ CriTok cri_window_token(const StreamView& s, int P, u32& cover, bool placing) {
    const int p = P + (int)threadIdx.x;
    const WinStarts w = window_starts(s, P, s.mask_word(P), cover);
    const bool lit = !w.start && (u32)p >= w.prev && p < s.n;
    return cri_token(w.start, lit, lit && placing ? (u32)s.src[p] : 0u, w.D, w.L);
}

__global__ __launch_bounds__(64) void enc_bits_cri_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                          const u32* __restrict__ index_list, u32 count, const mentry* __restrict__ match,
                                                          const u64* __restrict__ pos_off, alz_result* __restrict__ results, const u64* __restrict__ startmask) {
    __shared__ u32 buf[ALZ_CRI_WIN_DWORDS];
    if (blockIdx.x >= count) return;
    const int lane = (int)threadIdx.x;
    const StreamView s(src_base, dst_base, streams, index_list, pos_off, match, startmask, blockIdx.x);   // (src: the reversed source)
    u64 bits = 0; u32 cover = 0;
    for (int P = 0; P < s.n; P += 64) bits += (u64)__builtin_amdgcn_readlane((int)scan_add(cri_window_token(s, P, cover, false).width), 63);
    const u64 total = (bits + 7ull) >> 3;
    if (total > (u64)s.cap) { if (lane == 0) write_result(results, s.sid, 0u, s.src_len, ALZ_ST_OUTPUT_CAPACITY); return; }
    const u32 T = (u32)total;
    BitWindow<true, ALZ_CRI_WIN_DWORDS> w = { buf };
    cover = 0;
    for (int P = 0; P < s.n; P += 64) {
        const CriTok t = cri_window_token(s, P, cover, true);
        w.open(); w.sync();
        const u32 t0 = w.offset(t.width);
        if (t.width) w.put(t0, t.hv, t.hb);
        if (t.width > t.hb) w.put(t0 + t.hb + t.ones, t.tail, 8u);
        for (u64 lb = __ballot(t.ones != 0u); lb; lb &= lb - 1ull) w.fill_ones((int)__builtin_ctzll(lb), t0 + t.hb, t.ones);
        const u32 nfull = w.seal(), at = (u32)(w.G >> 3);
        for (u32 j = (u32)lane; j < nfull; j += 64u) { const u32 k = at + j; if (k < T) s.dst[T - 1u - k] = (u8)w.byte_at(j); }
        w.close();
    }
    if (lane == 0) {
        if (((u32)w.G & 7u) && (u32)(w.G >> 3) < T) s.dst[T - 1u - (u32)(w.G >> 3)] = (u8)w.carry;    // if (bitsLeft != 8) destination[dst--] = bitBuffer  :243-244
        write_result(results, s.sid, T, s.src_len, ALZ_ST_OK);
    }
}

// ---------------------------------------------------------------------------------------------- ALLZ written
// WriteALFlag  ALLZ.cs:160-173.  The managed sums are ints: with value < 2^30 (runs, lengths and distances of a source of at most 0x40000000
// bytes, minus one) the loop ends at bits <= 30 -- there bitMask + (1 << bits) - 1 = 2^31 - 2^startBits - 1 >= value --, every 1 << bits and
// every sum stays below 2^31, nothing wraps.
__device__ void allz_flag(FlagW& fw, int start, int value) {
    int mask = 0, bits = start;
    while (mask + ((1 << bits) - 1) < value) { bits++; mask = ((1 << (bits - start)) - 1) << start; fw.bit(1); }
    fw.bit(0);
    value -= mask;
    for (int i = 0; i < bits; i++) fw.bit((value >> i) & 1);                                // WriteInt: least significant bit first  FlagWriter.cs:90-98
}

// ---- ALLZ by the whole wavefront: a unit -- [run?][match] -- at the lane its match starts in.  What a unit writes is a function of the unit alone:
// the run bit, WriteALFlag(len_bits, run - 1), WriteALFlag(dist_bits, d - 1), WriteALFlag(copy_bits, l - 3); the run is the unit's side bytes, handed
// over right behind its own header.  Runs of more than eight bytes are copied by the whole wavefront.  Nothing is sized beforehand: every store is
// checked against the capacity and failure is reported by ballot.  Windows without a start bit are skipped.
// The end (:147-153): the bytes behind the last match are a last unit without a match; none left: a lone 1-bit.
// A unit has at most 1 + 61 + 39 + 39 bits and at least three positions: 22 units, 3 080 bits and the 7 carried in: 97 dwords, two more for a field's upper parts.
#define ALZ_ALLZ_WIN_DWORDS 128
// WriteALFlag(start, value) as `width` bits, least significant first  ALLZ.cs:160-173 (the int sums: see allz_flag above)
__device__ __forceinline__ u64 allz_field(int start, int value, u32& width) {
    int mask = 0, bits = start;
    while (mask + ((1 << bits) - 1) < value) { bits++; mask = ((1 << (bits - start)) - 1) << start; }
    const u32 ones = (u32)(bits - start);
    width = ones + 1u + (u32)bits;
    return ((1ull << ones) - 1ull) | ((u64)(u32)(value - mask) << (ones + 1u));
}

__global__ __launch_bounds__(64) void enc_bits_allz_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                           const u32* __restrict__ index_list, u32 count, const mentry* __restrict__ match,
                                                           const u64* __restrict__ pos_off, alz_result* __restrict__ results, const u64* __restrict__ startmask) {
    __shared__ u32 buf[ALZ_ALLZ_WIN_DWORDS];
    __shared__ u32 key[64], rsum[64];
    if (blockIdx.x >= count) return;
    const int lane = (int)threadIdx.x;
    const StreamView s(src_base, dst_base, streams, index_list, pos_off, match, startmask, blockIdx.x);
    const u8* src = s.src; u8* dst = s.dst; const u32 cap = s.cap;
    const int copy_bits = (int)(s.aux0 & 0xFFu), dist_bits = (int)((s.aux0 >> 8) & 0xFFu), len_bits = (int)((s.aux0 >> 16) & 0xFFu);
    BitWindow<false, ALZ_ALLZ_WIN_DWORDS> w = { buf };
    SidePlacer pl = { key, rsum, 0u };
    bool fail = false;
    auto store = [&](u32 at, u32 b) { if (at < cap) dst[at] = (u8)b; else fail = true; };
    // one window: this lane's unit (a run of `run` bytes from src + rs, then -- hasm -- the match d, l), or none
    auto window = [&](bool unit, u32 run, u32 rs, bool hasm, u32 d, u32 l) {
        u32 w0 = 0, w1 = 0, w2 = 0; u64 f0 = 0, f1 = 0, f2 = 0;
        if (unit && run) f0 = allz_field(len_bits, (int)run - 1, w0);
        if (unit && hasm) { f1 = allz_field(dist_bits, (int)d - 1, w1); f2 = allz_field(copy_bits, (int)l - 3, w2); }
        w.open();
        const u32 t0 = w.offset(unit ? 1u + w0 + w1 + w2 : 0u), hand = t0 + 1u + w0;   // hand: bits (from the window's first byte) when the run is handed over
        const u32 rat = pl.open(w, unit ? run : 0u, (hand + 7u) >> 3);
        w.sync();
        if (unit) {
            if (!run) w.put(t0, 1ull); else w.put(t0 + 1u, f0);                         // flag.WriteBit(false) + WriteALFlag | flag.WriteBit(true)  :139-150
            if (hasm) { w.put(t0 + 1u + w0, f1); w.put(t0 + 1u + w0 + w1, f2); }         // :155-156
        }
        if (unit && run && run <= 8u) { if (rat <= cap && run <= cap - rat) for (u32 i = 0; i < run; i++) dst[rat + i] = src[rs + i]; else fail = true; }
        for (u64 lb = __ballot(unit && run > 8u); lb; lb &= lb - 1ull) {
            const int l0 = (int)__builtin_ctzll(lb);
            const u32 o = (u32)__builtin_amdgcn_readlane((int)rat, l0), len = (u32)__builtin_amdgcn_readlane((int)run, l0), from = (u32)__builtin_amdgcn_readlane((int)rs, l0);
            if (o <= cap && len <= cap - o) for (u32 i = (u32)lane; i < len; i += 64u) dst[o + i] = src[from + i]; else fail = true;
        }
        close_placed(w, pl, store);
    };
    u32 cover = 0;                                                      // where the last match taken so far ends
    for (int P = 0; P < s.n; P += 64) {
        if ((P >> 6) >= s.nwords) break;
        const u64 mw = s.mask[P >> 6];
        if (mw == 0ull) continue;
        const WinStarts ws = window_starts(s, P, mw, cover);
        window(ws.start, ws.start ? (u32)(P + lane) - ws.prev : 0u, ws.prev, ws.start, ws.D, ws.L);
    }
    window(lane == 0, lane == 0 ? (u32)s.n - cover : 0u, cover, false, 0u, 0u);      // the bytes behind the last match; none: the lone 1-bit
    const u32 failed = __ballot(fail) != 0ull;
    if (lane == 0) {
        bool bad = failed != 0u;
        if (((u32)w.G & 7u) && !bad) { if (pl.carry_pos < cap) dst[pl.carry_pos] = (u8)w.carry; else bad = true; }
        const u64 total = ((w.G + 7ull) >> 3) + (u64)pl.rtot;
        if (total > (u64)cap) bad = true;
        write_result(results, s.sid, bad ? 0u : (u32)total, s.src_len, bad ? ALZ_ST_OUTPUT_CAPACITY : ALZ_ST_OK);
    }
}

// ALLZ.CompressHeaderless  :135-158 over FlagWriter(destination, Endian.Little).  A run goes straight to the output: with no flag byte open
// FlushIfNecessary lets it out at once; with one open the managed writer holds it back until the flag is complete and writes the flag in
// front -- FlagW has reserved that byte where the flag's first bit arrived, and nothing else reaches the output in between.
__device__ void allz_emit_lone(const u8* src, int n, Finder& mf, Out& out, u32 aux0) {
    const int copy_bits = (int)(aux0 & 0xFFu), dist_bits = (int)((aux0 >> 8) & 0xFFu), len_bits = (int)((aux0 >> 16) & 0xFFu);
    FlagW fw; fw.init(&out, false);
    int sp = 0;
    for (;;) {
        const Match mt = mf.next();
        const int plain = mt.offset - sp;
        if (plain > 0) {
            fw.bit(0);
            allz_flag(fw, len_bits, plain - 1);
            out.copy(src + sp, (u32)plain);
            sp += plain;
        } else fw.bit(1);
        if (sp == n) break;
        allz_flag(fw, dist_bits, mt.distance - 1);
        allz_flag(fw, copy_bits, mt.length - 3);
        sp += mt.length;
    }
    fw.flush();
}

// ---------------------------------------------------------------------------------------------- aPLib written
// LzChainMatchFinder over seven property sets (alz_encode_geometry), then source[0] raw and a FlagWriter(Endian.Big) stream of literals (0 + byte),
// one-byte matches (111 + 4 bits), short blocks (110 + byte), repeats (10, gamma 2, gamma L) and normal blocks (10, gamma high, low byte,
// gamma L - LengthDelta), an end marker (110 + byte 0).  A distance of exactly 1 << 21 arrives as 0 (m_pack21).  The branch `lengthDelta < 2 -> continue`
// (:256-259) is NOT here: every set's minimum length is at least LengthDelta + 2 over the set's distances -- set 1 (D <= 0x80, L 2..3) is a short block
// up to 0x7F and has delta 0 at 0x80; sets 0, 2..6 admit L >= 3, 4, .. >= 2 + delta -- so no (D, L) the finder returns reaches it
// (tests/test_apenc_cpu.py enumerates the edges).
__device__ __forceinline__ u32 ap_length_delta(u32 d) { return (d < 0x80u || d >= 0x7D00u) ? 2u : d >= 0x500u ? 1u : 0u; }   // LengthDelta  :288-295

// WriteGamma(v)  :309-319, bit by bit
__device__ void ap_gamma_lone(FlagW& fw, u32 v) {
    const int k = 32 - (int)__builtin_clz(v);
    for (int i = k - 2; i >= 0; i--) { fw.bit((int)((v >> i) & 1u)); fw.bit(i > 0); }
}

// CompressHeaderless  :185-285 token by token.  A payload byte enters FlagW where the managed code puts it into Buffer: in front of the bit that follows it (a
// literal, a short block, the end marker) or in front of FlushIfNecessary (a normal block's low byte).  With out.cap 0 nothing is stored and out.len counts: the sizing walk.
__device__ void aplib_emit_lone(const u8* src, int n, const mentry* m, const u64* mask, Out& out) {
    Finder mf = finder_over(m, mask, n);
    FlagW fw; fw.init(&out, true);
    int sp = 0; u32 last_offset = 0; bool lwm = false;
    out.put(src[sp++]);                                                                    // the first literal: raw  :191
    for (;;) {
        const Match mt = mf.next();
        int plain = mt.offset - sp;
        while (plain != 0) {
            plain--;
            const u32 by = src[sp++];
            lwm = false;
            int offset = -1;                                                                // a single-byte match  :205-219
            if (by == 0u) offset = 0;
            else {
                const int lookback = sp < 16 ? sp : 16;
                for (int i = 1; i < lookback; i++) if (src[sp - 1 - i] == by) { offset = i; break; }
            }
            if (offset != -1) { fw.bit(1); fw.bit(1); fw.bit(1); for (int i = 3; i >= 0; i--) fw.bit((offset >> i) & 1); continue; }
            fw.pay(by); fw.bit(0);                                                          // :231-232
        }
        if (mt.length == 0) break;
        const u32 D = m_dist21((u32)mt.distance), L = (u32)mt.length;
        if (!lwm && last_offset == D) {                                                     // repeat  :239-245
            fw.bit(1); fw.bit(0); ap_gamma_lone(fw, 2u); ap_gamma_lone(fw, L);
        } else if (L <= 3u && D <= 127u) {                                                  // short block  :246-252
            fw.bit(1); fw.bit(1); fw.pay((D << 1) | (L - 2u)); fw.bit(0);
        } else {                                                                            // normal block  :253-275 (lengthDelta >= 2: above)
            fw.bit(1); fw.bit(0);
            ap_gamma_lone(fw, (D >> 8) + 2u + (lwm ? 0u : 1u));
            fw.pay(D & 0xFFu); fw.flush_if_necessary();
            ap_gamma_lone(fw, L - ap_length_delta(D));
        }
        last_offset = D; lwm = true; sp += mt.length;
    }
    fw.bit(1); fw.bit(1); fw.pay(0); fw.bit(0);                                             // the end marker  :282-285
    fw.flush();
}

// ---- aPLib by the whole wavefront (position n is the end marker's).  A position is covered by a match (nothing), a one-byte match (7 bits), a literal
// (1 bit, 1 payload byte), a match's start (a repeat, a short block or a normal block: up to 2 + 26 + 60 bits, 0 or 1 payload byte) or the end (3 bits, 1 byte);
// which of the three a match is hangs on lwm and lastOffset, and those are local: lwm <=> the match before ended exactly here, lastOffset = its distance -- read
// from the lane of the window's start bit below this one, or carried in from the windows before as (end of the last match, its distance).  The 15-byte look-back
// is positional (source bytes, whatever covers them): two unaligned qwords, nearest equal byte first.
// The side bytes are the payload, one per lane at most, behind source[0].  With B the bits written when a payload byte enters Buffer it lands behind
// ceil((B + 1) / 8) flag bytes (a literal, a short block, the end: one more bit follows, and the flag byte that bit opens or completes goes in front) or
// ceil(B / 8) (a normal block's low byte: FlushIfNecessary) -- ApTok's kb says which.  A first walk over the same tokens adds up bits and payload: nothing is
// written unless the body fits.
// The bit string of a window: a match's start has at most 2 + 26 + 60 = 88 bits and is followed by a position it covers (a match has two bytes or more), a
// one-byte match has 7, a literal 1, the end 3: at most 32 starts of 88 bits -- 2 816 --, and the 7 carried in: 2 823 bits, 89 dwords and one for a field's low part.
#define ALZ_GAMMA_WIN_DWORDS 96
// WriteGamma(v) as `width` = 2 (bitlen(v) - 1) bits, most significant first: below the leading one every value bit, each followed by "more" (1) or "last" (0)  :309-319
__device__ __forceinline__ u64 ap_gamma(u32 v, u32& width) {
    const u32 k = 32u - (u32)__builtin_clz(v);
    width = 2u * (k - 1u);
    u64 x = v & ((1u << (k - 1u)) - 1u);                                 // (k - 1 <= 30 bits, spread to the even places)
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return (x << 1) | (0x5555555555555554ull & ((1ull << width) - 1ull));
}
// hb bits of hv, then tb bits of tv; a payload byte `pay` (has: kb != 0) that enters Buffer kb bits into the token -- with one more bit to follow (a literal 1, a short
// block or the end 3) or FlushIfNecessary (a normal block: kb = hb), which comes to the same place: behind ceil((B + kb) / 8) flag bytes
struct ApTok { u32 width, hv, hb, tb, kb, pay; u64 tv; };
// the token of this lane's position in the window at P; `cover`, `last_d`: where the last match taken so far ends, and its distance (0: none yet)
__device__ __forceinline__ ApTok ap_token(const StreamView& s, int P, u32& cover, u32& last_d) {
    ApTok t = { 0u, 0u, 0u, 0u, 0u, 0u, 0ull };
    const int lane = (int)threadIdx.x, p = P + lane, n = s.n;
    const u8* src = s.src;
    const u64 mw = s.mask_word(P);
    const u32 before = cover;
    const WinStarts w = window_starts(s, P, mw, cover);
    const u32 D = m_dist21(w.D), L = w.L, mend = w.start ? (u32)p + L : 0u;
    // the match before this lane's: the start bit below it in this window, or what the windows before left
    const u64 below = mw & ((1ull << lane) - 1ull);
    const int from = below ? 63 - (int)__builtin_clzll(below) : lane;
    u32 prev_end = (u32)__builtin_amdgcn_ds_bpermute(from << 2, (int)mend), prev_d = (u32)__builtin_amdgcn_ds_bpermute(from << 2, (int)D);
    if (!below) { prev_end = before; prev_d = last_d; }
    if (w.start) {
        const bool lwm = prev_end == (u32)p;
        if (!lwm && prev_d == D) {                                      // repeat: 10, gamma(2) = 00, gamma(L)  :239-245
            t.hv = 0x8u; t.hb = 4u; t.tv = ap_gamma(L, t.tb);
        } else if (L <= 3u && D <= 127u) {                              // short block: 11, the byte, 0  :246-252
            t.hv = 0x6u; t.hb = 3u; t.kb = 3u; t.pay = (D << 1) | (L - 2u);
        } else {                                                        // normal block: 10, gamma(high), the low byte, gamma(L - LengthDelta)  :253-275
            u32 gw; const u64 gh = ap_gamma((D >> 8) + 2u + (lwm ? 0u : 1u), gw);   // (high <= 0x2003: 26 bits)
            t.hv = (0x2u << gw) | (u32)gh; t.hb = 2u + gw; t.kb = t.hb; t.pay = D & 0xFFu;
            t.tv = ap_gamma(L - ap_length_delta(D), t.tb);
        }
    } else if (p == n) {                                                // the end marker: 11, byte 0, 0  :282-285
        t.hv = 0x6u; t.hb = 3u; t.kb = 3u;
    } else if (p >= 1 && p < n && (u32)p >= w.prev) {                   // a plain byte  :198-233 (position 0 went out raw)
        const u32 by = src[p];
        int off = -1;
        if (by == 0u) off = 0;
        else if (p >= 16) {                                             // the 15 bytes in front: p - 8 .. p - 1 and p - 16 .. p - 9, an exact zero-byte test on their XOR with the byte
            const u64 rep = 0x0101010101010101ull * by, lo7 = 0x7F7F7F7F7F7F7F7Full;
            const u64 za = load64(src + p - 8) ^ rep, zb = load64(src + p - 16) ^ rep;
            const u64 ea = ~(((za & lo7) + lo7) | za | lo7), eb = ~(((zb & lo7) + lo7) | zb | lo7) & ~0xFFull;   // (offset 16 is outside the look-back)
            if (ea) off = 1 + ((int)__builtin_clzll(ea) >> 3);
            else if (eb) off = 9 + ((int)__builtin_clzll(eb) >> 3);
        } else for (int i = 1; i <= p; i++) if (src[p - i] == by) { off = i; break; }     // min(16, srcPtr) at the stream's start  :210
        if (off >= 0) { t.hv = 0x70u | (u32)off; t.hb = 7u; }           // 111 + 4 bits  :223-226
        else { t.hb = 1u; t.kb = 1u; t.pay = by; }                      // the byte, then 0  :231-232
    }
    t.width = t.hb + t.tb;
    if (mw) last_d = (u32)__builtin_amdgcn_readlane((int)D, 63 - (int)__builtin_clzll(mw));
    return t;
}

__global__ __launch_bounds__(64) void enc_gamma_ap_kernel(const u8* __restrict__ src_base, u8* __restrict__ dst_base, const alz_stream* __restrict__ streams,
                                                          const u32* __restrict__ index_list, u32 count, const mentry* __restrict__ match,
                                                          const u64* __restrict__ pos_off, alz_result* __restrict__ results, const u64* __restrict__ startmask) {
    __shared__ u32 buf[ALZ_GAMMA_WIN_DWORDS];
    __shared__ u32 key[64], rsum[64];
    if (blockIdx.x >= count) return;
    const int lane = (int)threadIdx.x;
    const StreamView s(src_base, dst_base, streams, index_list, pos_off, match, startmask, blockIdx.x);
    // the sizing walk: source[0], the flag bytes, the payload
    u64 bits = 0; u32 npay = 0, cover = 0, last_d = 0;
    for (int P = 0; P <= s.n; P += 64) {
        const ApTok t = ap_token(s, P, cover, last_d);
        bits += (u64)__builtin_amdgcn_readlane((int)scan_add(t.width), 63);
        npay += (u32)__popcll(__ballot(t.kb != 0u));
    }
    const u64 total = 1ull + ((bits + 7ull) >> 3) + (u64)npay;
    if (total > (u64)s.cap) { if (lane == 0) write_result(results, s.sid, 0u, s.src_len, ALZ_ST_OUTPUT_CAPACITY); return; }
    if (lane == 0) s.dst[0] = s.src[0];                                 // :191
    BitWindow<true, ALZ_GAMMA_WIN_DWORDS> w = { buf };
    SidePlacer pl = { key, rsum, 1u };
    cover = 0; last_d = 0;
    auto store = [&](u32 at, u32 b) { if (at < s.cap) s.dst[at] = (u8)b; };  // (the body fits: the test costs nothing and no index is trusted)
    for (int P = 0; P <= s.n; P += 64) {
        const ApTok t = ap_token(s, P, cover, last_d);
        w.open();
        const u32 t0 = w.offset(t.width);
        const bool has = t.kb != 0u;
        const u32 pat = pl.open(w, has ? 1u : 0u, (t0 + t.kb + 7u) >> 3);
        w.sync();
        if (t.hb) w.put(t0, t.hv, t.hb);
        if (t.tb > 32u) { w.put(t0 + t.hb, (u32)(t.tv >> 32), t.tb - 32u); w.put(t0 + t.hb + t.tb - 32u, (u32)t.tv, 32u); }
        else if (t.tb) w.put(t0 + t.hb, (u32)t.tv, t.tb);
        if (has) store(pat, t.pay);
        close_placed(w, pl, store);
    }
    if (lane == 0) {
        if ((u32)w.G & 7u) store(pl.carry_pos, w.carry);                // Dispose: the open flag byte  FlagWriter.cs:111-127
        write_result(results, s.sid, (u32)total, s.src_len, ALZ_ST_OK);
    }
}
