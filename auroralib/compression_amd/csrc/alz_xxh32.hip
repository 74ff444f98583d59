// alz_xxh32.hip -- XXH32 of byte ranges in HBM (alz_xxh32_batch*), and the range copy of the batched LZ4 / Snappy file layer.
//
// XXH32 is not linear: v = rotl(v + w * P2, 13) * P1 over the dwords w of an accumulator's column cannot be joined from partial results, so
// one range is a serial chain over its 16-byte stripes.  What is parallel is the four accumulators and the ranges:
//
//   xxh32 kernel  FOUR LANES per range, 16 ranges per wavefront.  Lane j of a group owns accumulator v_j and reads dword j of every stripe:
//                 a group's four loads are one stripe.  ALZ_XXH32_UNROLL stripes per iteration, their loads issued in front of the multiply
//                 chain.  A range that starts at an odd byte is read in ALIGNED dwords -- the one that holds the first byte of the lane's
//                 word and, unless the range is dword-aligned, the one behind it -- and the word is funnel-shifted out of the pair.  Every
//                 dword loaded holds a byte of the range.  Behind the stripes every lane of the group folds the four accumulators (a
//                 butterfly over the quad) and runs the tail -- length, up to three dwords, up to three bytes, avalanche -- on words the
//                 group loaded the same way; lane 0 stores.  Groups of different lengths diverge: a group that is done idles.
//                 No LDS, no table.
//   copy kernel   a list of (src_off, dst_off, n): ONE WAVEFRONT per piece of ALZ_COPY_PIECE bytes of a range, the grid over all pieces of
//                 all ranges.  A piece is written as aligned 16-byte stores (lane l stores granules l, l + 64, ...), the bytes in front
//                 of the first and behind the last granule one by one; the source of a granule is read in aligned dwords and
//                 funnel-shifted (one 16-byte load where source and destination are aligned alike).
#include "alz_xxh32.h"

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;

__device__ __forceinline__ u32 rotl(u32 x, u32 r) { return (x << r) | (x >> (32u - r)); }                 // 0 < r < 32
// the dword that starts `sh` bytes into lo (sh < 4; hi is the dword behind lo): one byte-align / bit-align instruction
__device__ __forceinline__ u32 funnel(u32 hi, u32 lo, u32 sh) { return (u32)((((u64)hi << 32) | lo) >> (8u * sh)); }

}   // namespace

__global__ __launch_bounds__(256) void alz_xxh32_kernel(const u8* __restrict__ src, const alz_stream* __restrict__ ranges, u32 n, u32 seed,
                                                        u32* __restrict__ out) {
    const u32 t = blockIdx.x * 256u + threadIdx.x, r = t >> 2, j = t & 3u, lane = threadIdx.x & 63u;
    const bool valid = r < n;
    const u32 len = valid ? ranges[r].src_len : 0u;
    const uintptr_t p = (uintptr_t)src + (valid ? ranges[r].src_off : 0u);
    const u32 sh = (u32)(p & 3u), step = sh ? 1u : 0u;                          // an aligned range never looks at the dword behind its word
    const u32* q = (const u32*)(p & ~(uintptr_t)3) + j;                         // the dword that holds the first byte of this lane's word
    const u32 S = len >> 4;
    u32 v = seed + (j == 0 ? P1 + P2 : j == 1 ? P2 : j == 2 ? 0u : 0u - P1);
    u32 s = 0;
    for (; s + ALZ_XXH32_UNROLL <= S; s += ALZ_XXH32_UNROLL, q += 4u * ALZ_XXH32_UNROLL) {
        u32 lo[ALZ_XXH32_UNROLL], hi[ALZ_XXH32_UNROLL];
#pragma unroll
        for (u32 u = 0; u < ALZ_XXH32_UNROLL; u++) { lo[u] = q[4u * u]; hi[u] = q[4u * u + step]; }
#pragma unroll
        for (u32 u = 0; u < ALZ_XXH32_UNROLL; u++) v = rotl(v + funnel(hi[u], lo[u], sh) * P2, 13) * P1;
    }
    for (; s < S; s++, q += 4) v = rotl(v + funnel(q[step], q[0], sh) * P2, 13) * P1;

    // the tail: bytes [sh, sh + rem) of the aligned dwords from q - j on; dword k holds one of them when 4 k < sh + rem
    const u32 rem = len & 15u, span = rem ? sh + rem : 0u;
    const u32 tlo = 4u * j < span ? q[0] : 0u, thi = (sh && 4u * (j + 1u) < span) ? q[1] : 0u;
    const u32 w = funnel(thi, tlo, sh);
    const u32 base = lane & ~3u;
    const u32 w0 = __shfl(w, base, 64), w1 = __shfl(w, base + 1u, 64), w2 = __shfl(w, base + 2u, 64), w3 = __shfl(w, base + 3u, 64);
    u32 h = rotl(v, j == 0 ? 1u : j == 1 ? 7u : j == 2 ? 12u : 18u);
    h += __shfl_xor(h, 1, 64);
    h += __shfl_xor(h, 2, 64);
    if (S == 0) h = seed + P5;
    h += len;
    const u32 nw = rem >> 2, nb = rem & 3u;
    if (nw > 0) h = rotl(h + w0 * P3, 17) * P4;
    if (nw > 1) h = rotl(h + w1 * P3, 17) * P4;
    if (nw > 2) h = rotl(h + w2 * P3, 17) * P4;
    const u32 last = nw == 0 ? w0 : nw == 1 ? w1 : nw == 2 ? w2 : w3;
    if (nb > 0) h = rotl(h + (last & 0xFFu) * P5, 11) * P1;
    if (nb > 1) h = rotl(h + ((last >> 8) & 0xFFu) * P5, 11) * P1;
    if (nb > 2) h = rotl(h + ((last >> 16) & 0xFFu) * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    if (valid && j == 0) out[r] = h;
}

__global__ __launch_bounds__(256) void alz_range_copy_kernel(const u8* __restrict__ src, u8* __restrict__ dst, const alz_copy_range* __restrict__ ranges,
                                                             u32 n, u32 pieces) {
    const u32 lane = threadIdx.x & 63u;
    const u32 g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (g >= pieces) return;
    u32 lo = 0, hi = n;                                                         // the last range with first <= g: it has piece g (an empty range shares its `first` with the one behind it)
    while (hi - lo > 1) {
        const u32 mid = lo + (hi - lo) / 2;
        if (ranges[mid].first <= g) lo = mid; else hi = mid;
    }
    const alz_copy_range R = ranges[lo];
    const u64 off = (u64)(g - R.first) * ALZ_COPY_PIECE;
    const u32 left = (u32)(R.n - off), L = left < ALZ_COPY_PIECE ? left : ALZ_COPY_PIECE;
    const u8* s = src + R.src_off + off;
    u8* d = dst + R.dst_off + off;
    u32 head = (16u - (u32)((uintptr_t)d & 15u)) & 15u;
    if (head > L) head = L;
    const u32 body = (L - head) >> 4, tail = L - head - 16u * body;
    if (lane < head) d[lane] = s[lane];
    if (lane < tail) d[L - tail + lane] = s[L - tail + lane];
    const u8* sb = s + head;
    u8* db = d + head;
    if (((uintptr_t)sb & 15u) == 0) {
        for (u32 q = lane; q < body; q += 64u) *(uint4*)(db + 16u * q) = *(const uint4*)(sb + 16u * q);
        return;
    }
    const u32 sh = (u32)((uintptr_t)sb & 3u);
    const u32* sq = (const u32*)((uintptr_t)sb & ~(uintptr_t)3);
    for (u32 q = lane; q < body; q += 64u) {
        const u32* a = sq + 4u * q;
        const u32 d0 = a[0], d1 = a[1], d2 = a[2], d3 = a[3], d4 = a[sh ? 4 : 3];   // (aligned to a dword: the fifth holds no byte of the granule)
        *(uint4*)(db + 16u * q) = make_uint4(funnel(d1, d0, sh), funnel(d2, d1, sh), funnel(d3, d2, sh), funnel(d4, d3, sh));
    }
}

hipError_t alz_launch_xxh32(hipStream_t stream, uint32_t seed, const void* d_src, const alz_stream* d_ranges, uint32_t n, uint32_t* d_out) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_xxh32_kernel, dim3((n + 63u) / 64u), dim3(256), 0, stream, (const u8*)d_src, d_ranges, n, seed, d_out);
    return hipGetLastError();
}

hipError_t alz_launch_range_copy(hipStream_t stream, const void* d_src, void* d_dst, const alz_copy_range* d_ranges, uint32_t n, uint32_t pieces) {
    if (n == 0 || pieces == 0) return hipSuccess;
    hipLaunchKernelGGL(alz_range_copy_kernel, dim3((pieces + 3u) / 4u), dim3(256), 0, stream, (const u8*)d_src, (u8*)d_dst, d_ranges, n, pieces);
    return hipGetLastError();
}
