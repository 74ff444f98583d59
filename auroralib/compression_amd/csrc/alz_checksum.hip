// alz_checksum.hip -- Adler-32, CRC-32 and CRC-32C of byte ranges in HBM (alz_checksum_batch*, alz_crc32c_batch*).  Two launches per batch:
//
//   chunk kernel  every range is cut into chunks of `chunk` bytes; ONE WAVEFRONT sums one chunk, four wavefronts to a workgroup, the grid
//                 over all chunks of all ranges -- 10 000 ranges of 256 KiB and one range of 1 GiB fill the GPU alike.  A chunk is read in
//                 aligned 16-byte granules, lane l taking granules l, l + 64, ...: one wavefront load is 1 KiB of consecutive bytes.  Only
//                 granules that hold a byte of the chunk are loaded; the bytes of the first and last granule outside it are masked to 0.
//   fold kernel   one wavefront per range joins the range's chunk sums (alz_checksum_join, the code of alz_checksum_combine): every lane a
//                 run of neighbouring chunks, then a tree over the lanes.
//
// Adler-32 of bytes d_0 .. d_(L-1): A = 1 + sum d_j, B = L + sum (L - j) d_j, both mod 65521.  A lane keeps three plain 32-bit sums over its
// granules (the bytes of a granule, the bytes weighted by their place in the granule, the byte sums weighted by the round) and reduces them
// once, behind the chunk: with at most ALZ_CHECKSUM_CHUNK_MAX = 1 MiB to a chunk (1 025 rounds) the largest is 4 080 * 1 025 * 1 026 / 2 <
// 2^32.  The places count from the first granule; the head h of that granule in front of the chunk is taken out at the end.
// A CRC (CRC-32 and CRC-32C differ in the polynomial P alone: alz_checksum_poly) is linear over GF(2): a lane carries the raw CRC (start value 0) of ITS granules, acc = acc x^8192 + g0 x^128 + g1 x^96 + g2 x^64 +
// g3 x^32 mod P per round (its next granule lies 1 KiB = 8 192 bits on).  The five multipliers are constants, so each product is 32 steps of
// "coefficient set ? xor a literal" in the vector ALU -- no table, no LDS.  Behind the chunk a lane multiplies by x^(8 e), e the bytes between
// the end of its last granule and the end of the chunk (-15 .. 1 008: a table of x^(8 i), i = e + 15, and one multiplication by x^-120), and
// the lanes' values are xor-ed.  Start value and final inversion are applied once per range, in the fold kernel.
#include "alz_checksum.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kM = ALZ_ADLER_BASE;

template <u32 P> constexpr bool order_holds() { return alz_crc_mul<P>(alz_crc_xinv120<P>(), alz_crc_xpow_c<P>(120)) == ALZ_CRC_ONE; }
static_assert(order_holds<ALZ_CRC_POLY>() && order_holds<ALZ_CRC32C_POLY>(), "x^order is not 1 modulo a CRC polynomial (alz_crc_order)");

__device__ const alz_crc_xbyte_table<ALZ_CRC_POLY> kXByte{};
__device__ const alz_crc_xbyte_table<ALZ_CRC32C_POLY> kXByteC{};
template <u32 P> __device__ __forceinline__ u32 xbyte(int i) { return P == ALZ_CRC32C_POLY ? kXByteC.v[i] : kXByte.v[i]; }

// a K mod P for a constant K: unrolled, the 32 multiples of K fold to literals
template <u32 P, u32 K>
__device__ __forceinline__ u32 mul_const(u32 a) {
    u32 p = 0, b = K;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        p ^= (u32)((int32_t)(a << j) >> 31) & b;
        b = alz_crc_xtime<P>(b);
    }
    return p;
}

__device__ __forceinline__ u32 byte_mask(int k) { return k <= 0 ? 0u : k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u; }   // the low k bytes
// keep bytes [lo, hi) of a granule
__device__ __forceinline__ void mask_granule(u32 (&d)[4], int lo, int hi) {
#pragma unroll
    for (int w = 0; w < 4; w++) d[w] &= byte_mask(hi - 4 * w) & ~byte_mask(lo - 4 * w);
}

__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u32 wave_xor(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= __shfl_xor(v, o, 64);
    return v;
}

// the last range r < n with first[r] <= g (empty ranges share their `first` with the range behind them); g < first[n]
__device__ __forceinline__ u32 range_of_chunk(const u32* __restrict__ first, u32 n, u32 g) {
    u32 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (first[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// partial[g]: Adler-32 of chunk g, or its raw CRC (start value 0, no final inversion).  KIND: an alz_checksum_kind or ALZ_CK_CRC32C.
template <u32 KIND>
__device__ __forceinline__ void chunk_body(const u8* __restrict__ src, const alz_stream* __restrict__ ranges, u32 n,
                                           const u32* __restrict__ first, u32 total, u32 chunk, u32* __restrict__ partial) {
    constexpr u32 P = alz_checksum_poly(KIND);
    const u32 lane = threadIdx.x & 63u;
    const u32 g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (g >= total) return;
    const u32 r = range_of_chunk(first, n, g);
    const u64 off = (u64)(g - first[r]) * chunk;                                // < src_len: the chunk exists
    const u64 left = (u64)ranges[r].src_len - off;
    const u32 L = left < chunk ? (u32)left : chunk;
    const uintptr_t p = (uintptr_t)src + ranges[r].src_off + off;
    const uintptr_t a0 = p & ~(uintptr_t)15;
    const u32 h = (u32)(p - a0), span = h + L, Q = (span + 15u) >> 4;           // the chunk is bytes [h, span) of granules 0 .. Q - 1
    if (KIND == ALZ_CK_ADLER32) {
        u32 t1 = 0, t2 = 0, t3 = 0, round = 0;
        for (u32 q = lane; q < Q; q += 64u, round++) {
            const uint4 v = *(const uint4*)(a0 + (uintptr_t)q * 16u);
            u32 d[4] = {v.x, v.y, v.z, v.w};
            const int lo = q == 0 ? (int)h : 0, hi = (int)(span - q * 16u);
            if (lo != 0 || hi < 16) mask_granule(d, lo, hi);
            u32 s1 = 0, s2 = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const u32 b0 = d[w] & 0xFFu, b1 = (d[w] >> 8) & 0xFFu, b2 = (d[w] >> 16) & 0xFFu, b3 = d[w] >> 24;
                const u32 s = b0 + b1 + b2 + b3;
                s1 += s;
                s2 += 4u * w * s + b1 + 2u * b2 + 3u * b3;
            }
            t1 += s1; t2 += s2; t3 += round * s1;
        }
        // place of a byte, from the first granule: 16 (64 round + lane) + k
        const u32 r1 = t1 % kM;
        const u32 sum1 = wave_sum(r1), sum2 = wave_sum(t2 % kM), sum3 = wave_sum(t3 % kM), suml = wave_sum(lane * r1);
        if (lane == 0) {
            const u64 s1 = sum1 % kM;
            const u64 wp = (16u * (64u * (u64)(sum3 % kM) + suml) + sum2) % kM;
            const u64 w = (wp + kM - (h * s1) % kM) % kM;                       // sum j d_j, j from the start of the chunk
            const u64 lm = L % kM;
            const u64 a = (1u + s1) % kM, b = (lm * (1u + s1) + kM - w) % kM;   // L + L sum d - sum j d
            partial[g] = (u32)((b << 16) | a);
        }
    } else {
        u32 acc = 0, q = lane;
        for (; q < Q; q += 64u) {
            const uint4 v = *(const uint4*)(a0 + (uintptr_t)q * 16u);
            u32 d[4] = {v.x, v.y, v.z, v.w};
            const int lo = q == 0 ? (int)h : 0, hi = (int)(span - q * 16u);
            if (lo != 0 || hi < 16) mask_granule(d, lo, hi);
            acc = mul_const<P, alz_crc_xpow_c<P>(8192)>(acc) ^ mul_const<P, alz_crc_xpow_c<P>(128)>(d[0]) ^ mul_const<P, alz_crc_xpow_c<P>(96)>(d[1]) ^
                  mul_const<P, alz_crc_xpow_c<P>(64)>(d[2]) ^ mul_const<P, alz_crc_xpow_c<P>(32)>(d[3]);
        }
        u32 mine = 0;
        if (q != lane) {                                                        // granule q - 64 was this lane's last: it ends at byte 16 (q - 63)
            const int e = (int)span - (int)(16u * (q - 63u));                   // -15 .. 1 008
            mine = alz_crc_mul<P>(acc, xbyte<P>(e + 15));
        }
        const u32 all = wave_xor(mine);
        if (lane == 0) partial[g] = alz_crc_mul<P>(all, alz_crc_xinv120<P>());
    }
}

// out[r]: the checksum of range r from its chunks' partial sums
template <u32 KIND>
__device__ __forceinline__ void fold_body(const alz_stream* __restrict__ ranges, const u32* __restrict__ first, u32 chunk,
                                          const u32* __restrict__ partial, u32* __restrict__ out) {
    constexpr u32 P = alz_checksum_poly(KIND);
    constexpr bool CRC = KIND != ALZ_CK_ADLER32;
    const u32 r = blockIdx.x, lane = threadIdx.x;
    const u32 f = first[r], C = first[r + 1] - f, len = ranges[r].src_len;
    const u32 m = (C + 63u) / 64u;                                              // chunks per lane, in order
    const u32 c0 = lane * m < C ? lane * m : C, c1 = c0 + m < C ? c0 + m : C;
    const u32 xck = CRC ? alz_crc_xpow_bytes<P>(chunk) : 0u;
    u32 v = alz_checksum_empty(KIND), bytes = 0;
    for (u32 c = c0; c < c1; c++) {
        const u64 left = (u64)len - (u64)c * chunk;
        const u32 cl = left < chunk ? (u32)left : chunk;
        v = alz_checksum_join(KIND, v, partial[f + c], cl, !CRC || cl == chunk ? xck : alz_crc_xpow_bytes<P>(cl));
        bytes += cl;
    }
    const u32 used = m ? (C + m - 1u) / m : 0u;                                 // lanes that hold chunks
    for (u32 o = 1; o < used; o <<= 1) {
        const u32 pv = __shfl_down(v, o, 64), pb = __shfl_down(bytes, o, 64);
        const u32 j = alz_checksum_join(KIND, v, pv, pb, CRC ? alz_crc_xpow_bytes<P>(pb) : 0u);
        if ((lane & (2u * o - 1u)) == 0 && lane + o < 64u) { v = j; bytes += pb; }
    }
    if (lane == 0) out[r] = CRC ? v ^ alz_crc_mul<P>(0xFFFFFFFFu, alz_crc_xpow_bytes<P>(len)) ^ 0xFFFFFFFFu : v;
}

}   // namespace

template <u32 KIND>
__global__ __launch_bounds__(256) void alz_checksum_chunk_kernel(const u8* __restrict__ src, const alz_stream* __restrict__ ranges, u32 n,
                                                                 const u32* __restrict__ first, u32 total, u32 chunk, u32* __restrict__ partial) {
    chunk_body<KIND>(src, ranges, n, first, total, chunk, partial);
}
template <u32 KIND>
__global__ __launch_bounds__(64) void alz_checksum_fold_kernel(const alz_stream* __restrict__ ranges, const u32* __restrict__ first, u32 chunk,
                                                               const u32* __restrict__ partial, u32* __restrict__ out) {
    fold_body<KIND>(ranges, first, chunk, partial, out);
}
// CRC-32C: the same two bodies over the Castagnoli polynomial, as kernels with names of their own
__global__ __launch_bounds__(256) void alz_crc32c_chunk_kernel(const u8* __restrict__ src, const alz_stream* __restrict__ ranges, u32 n,
                                                               const u32* __restrict__ first, u32 total, u32 chunk, u32* __restrict__ partial) {
    chunk_body<ALZ_CK_CRC32C>(src, ranges, n, first, total, chunk, partial);
}
__global__ __launch_bounds__(64) void alz_crc32c_fold_kernel(const alz_stream* __restrict__ ranges, const u32* __restrict__ first, u32 chunk,
                                                             const u32* __restrict__ partial, u32* __restrict__ out) {
    fold_body<ALZ_CK_CRC32C>(ranges, first, chunk, partial, out);
}

hipError_t alz_launch_checksum(uint32_t kind, hipStream_t stream, const void* d_src, const alz_stream* d_ranges, uint32_t n,
                               const uint32_t* d_first, uint32_t total_chunks, uint32_t chunk, uint32_t* d_partial, uint32_t* d_out) {
    if (kind > ALZ_CK_CRC32C || chunk == 0 || chunk % 1024u || chunk > ALZ_CHECKSUM_CHUNK_MAX) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (total_chunks) {
        const dim3 grid((total_chunks + 3u) / 4u), block(256);
        if (kind == ALZ_CK_CRC32C) hipLaunchKernelGGL(alz_crc32c_chunk_kernel, grid, block, 0, stream, (const u8*)d_src, d_ranges, n, d_first, total_chunks, chunk, d_partial);
        else if (kind == ALZ_CK_CRC32) hipLaunchKernelGGL(alz_checksum_chunk_kernel<ALZ_CK_CRC32>, grid, block, 0, stream, (const u8*)d_src, d_ranges, n, d_first, total_chunks, chunk, d_partial);
        else hipLaunchKernelGGL(alz_checksum_chunk_kernel<ALZ_CK_ADLER32>, grid, block, 0, stream, (const u8*)d_src, d_ranges, n, d_first, total_chunks, chunk, d_partial);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (kind == ALZ_CK_CRC32C) hipLaunchKernelGGL(alz_crc32c_fold_kernel, dim3(n), dim3(64), 0, stream, d_ranges, d_first, chunk, d_partial, d_out);
    else if (kind == ALZ_CK_CRC32) hipLaunchKernelGGL(alz_checksum_fold_kernel<ALZ_CK_CRC32>, dim3(n), dim3(64), 0, stream, d_ranges, d_first, chunk, d_partial, d_out);
    else hipLaunchKernelGGL(alz_checksum_fold_kernel<ALZ_CK_ADLER32>, dim3(n), dim3(64), 0, stream, d_ranges, d_first, chunk, d_partial, d_out);
    return hipGetLastError();
}
