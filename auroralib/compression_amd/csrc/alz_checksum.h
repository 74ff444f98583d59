// alz_checksum.h -- Adler-32 (RFC 1950), CRC-32 (polynomial 0xEDB88320, as zlib.crc32) and CRC-32C (0x82F63B78, Castagnoli) over byte
// ranges in HBM: the launcher of alz_checksum.hip for the host TU, and the arithmetic that joins the checksums of two neighbouring pieces.
// That arithmetic is __host__ __device__: alz_checksum_combine / alz_crc32c_combine (host) and the fold kernels (device) run the same code.
// Not part of the ABI (include/auroralz.h: alz_checksum_batch*, alz_checksum_combine, alz_crc32c_batch*, alz_crc32c_combine).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#ifndef ALZ_CHECKSUM_CHUNK
#define ALZ_CHECKSUM_CHUNK 32768u    /* bytes of a range one wavefront sums (docs/EXPERIMENTS.md 17 holds the ladder) */
#endif
#define ALZ_CHECKSUM_CHUNK_MAX (1u << 20)   /* the Adler kernel's 32-bit lane sums are exact up to here (alz_checksum.hip) */

#define ALZ_ADLER_BASE 65521u
#define ALZ_CRC_POLY 0xEDB88320u     /* CRC-32 (zlib.crc32) */
#define ALZ_CRC32C_POLY 0x82F63B78u  /* CRC-32C (Castagnoli): the checksum of the framed Snappy container */
#define ALZ_CK_CRC32C 2u             /* a kind of the launcher only: the public alz_checksum_batch* refuse it, alz_crc32c_batch* pass it */

// ---- a CRC as polynomials over GF(2) modulo P, in the bit order of the CRC register: bit 31 is x^0, bit 0 is x^31 ("reflected").  The
// register after a message M from the start value 0 is M(x) x^32 mod P (the "raw" CRC); it is linear in M, so raw(A || B) =
// raw(A) x^(8 len B) + raw(B), and the same holds for the finished CRCs of A, B and A || B (zlib's crc32_combine).  Every helper takes the
// reflected polynomial P as a template argument; without one it is CRC-32's.
#define ALZ_CRC_ONE 0x80000000u                                                 /* x^0 */
template <uint32_t P = ALZ_CRC_POLY>
__host__ __device__ constexpr uint32_t alz_crc_xtime(uint32_t a) { return (a >> 1) ^ ((a & 1u) ? P : 0u); }   // a x mod P
// a b mod P, 32 fixed steps (no data-dependent branch: every lane of a wavefront takes the same path)
template <uint32_t P = ALZ_CRC_POLY>
__host__ __device__ constexpr uint32_t alz_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int j = 0; j < 32; j++) {
        p ^= (uint32_t)((int32_t)(a << j) >> 31) & b;                           // coefficient j of a is bit 31 - j
        b = alz_crc_xtime<P>(b);
    }
    return p;
}
// x^(2^k) mod P for k < 32, by squaring
template <uint32_t P = ALZ_CRC_POLY>
struct alz_crc_squares {
    uint32_t v[32];
    constexpr alz_crc_squares() : v{} {
        uint32_t p = ALZ_CRC_ONE >> 1;                                          // x^1
        for (int k = 0; k < 32; k++) { v[k] = p; p = alz_crc_mul<P>(p, p); }
    }
};
// A multiple of the order of x modulo P: exponents count modulo it.  CRC-32's polynomial is primitive (2^32 - 1); CRC-32C's is x + 1 times
// a primitive polynomial of degree 31 (2^31 - 1).  alz_checksum.hip checks x^order = 1 at compile time.
template <uint32_t P> constexpr uint64_t alz_crc_order() { return P == ALZ_CRC32C_POLY ? 0x7FFFFFFFull : 0xFFFFFFFFull; }
// x^n mod P
template <uint32_t P = ALZ_CRC_POLY>
__host__ __device__ inline uint32_t alz_crc_xpow(uint64_t n) {
    static constexpr alz_crc_squares<P> sq;
    n %= alz_crc_order<P>();
    uint32_t p = ALZ_CRC_ONE;
    for (int k = 0; n; n >>= 1, k++)
        if (n & 1u) p = alz_crc_mul<P>(sq.v[k], p);
    return p;
}
template <uint32_t P = ALZ_CRC_POLY>
__host__ __device__ inline uint32_t alz_crc_xpow_bytes(uint64_t len) { return alz_crc_xpow<P>((len % alz_crc_order<P>()) * 8u); }   // x^(8 len)
// x^n mod P at compile time
template <uint32_t P = ALZ_CRC_POLY>
constexpr uint32_t alz_crc_xpow_c(uint64_t n) {
    uint32_t p = ALZ_CRC_ONE, s = ALZ_CRC_ONE >> 1;
    while (n) { if (n & 1u) p = alz_crc_mul<P>(p, s); s = alz_crc_mul<P>(s, s); n >>= 1; }
    return p;
}
// x^(8 i), i < 1024
template <uint32_t P = ALZ_CRC_POLY>
struct alz_crc_xbyte_table {
    uint32_t v[1024];
    constexpr alz_crc_xbyte_table() : v{} {
        uint32_t p = ALZ_CRC_ONE;
        for (int i = 0; i < 1024; i++) { v[i] = p; for (int k = 0; k < 8; k++) p = alz_crc_xtime<P>(p); }
    }
};
// x^-120
template <uint32_t P = ALZ_CRC_POLY>
constexpr uint32_t alz_crc_xinv120() { return alz_crc_xpow_c<P>(alz_crc_order<P>() - 120u); }

// ---- the CRC of A || B from those of A and of B; `xb` is x^(8 len_b) mod P (alz_crc_xpow_bytes<P>): a caller that joins many pieces of
// one length computes it once.  alz_checksum_combine / alz_crc32c_combine (host) and the fold kernels (device) run this.
template <uint32_t P>
__host__ __device__ inline uint32_t alz_crc_join(uint32_t a, uint32_t b, uint32_t xb) { return alz_crc_mul<P>(a, xb) ^ b; }
// the polynomial of a CRC kind (0 for Adler-32)
__host__ __device__ constexpr uint32_t alz_checksum_poly(uint32_t kind) { return kind == ALZ_CK_CRC32 ? ALZ_CRC_POLY : kind == ALZ_CK_CRC32C ? ALZ_CRC32C_POLY : 0u; }

// ---- the checksum of A || B from those of A and of B.  `xb`: as above, for the CRC kinds only.
__host__ __device__ inline uint32_t alz_checksum_join(uint32_t kind, uint32_t a, uint32_t b, uint64_t len_b, uint32_t xb) {
    if (kind == ALZ_CK_CRC32) return alz_crc_join<ALZ_CRC_POLY>(a, b, xb);
    if (kind == ALZ_CK_CRC32C) return alz_crc_join<ALZ_CRC32C_POLY>(a, b, xb);
    // Adler-32: A = 1 + sum d, B = sum over the prefixes of A.  Behind len_b more bytes A(A||B) = A1 + A2 - 1 and every one of those
    // prefixes starts from A1 instead of 1: B(A||B) = B1 + B2 + len_b (A1 - 1).
    const uint64_t M = ALZ_ADLER_BASE;
    const uint64_t a1 = a & 0xFFFFu, b1 = a >> 16, a2 = b & 0xFFFFu, b2 = b >> 16;
    const uint64_t lo = (a1 + a2 + M - 1u) % M;
    const uint64_t hi = (b1 + b2 + (len_b % M) * ((a1 + M - 1u) % M)) % M;
    return (uint32_t)((hi << 16) | lo);
}
__host__ __device__ inline uint32_t alz_checksum_empty(uint32_t kind) { return kind == ALZ_CK_ADLER32 ? 1u : 0u; }   // of no bytes

// One batch: `first` holds n + 1 words, the number of chunks in front of range i (first[n] = all of them); a range of src_len bytes has
// ceil(src_len / chunk) chunks.  d_partial: first[n] words of scratch.  Two launches: every chunk's checksum, then one wavefront per range
// joins that range's.  d_out[i] is the checksum of range i.  chunk: a multiple of 1024, at most ALZ_CHECKSUM_CHUNK_MAX.  kind: an
// alz_checksum_kind or ALZ_CK_CRC32C.
hipError_t alz_launch_checksum(uint32_t kind, hipStream_t stream, const void* d_src, const alz_stream* d_ranges, uint32_t n,
                               const uint32_t* d_first, uint32_t total_chunks, uint32_t chunk, uint32_t* d_partial, uint32_t* d_out);
