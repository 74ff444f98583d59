// crc_lane_model.cpp -- a host model of the lane arithmetic of the CRC chunk and fold kernels (csrc/alz_checksum.hip), over the very GF(2)
// helpers of csrc/alz_checksum.h, for both polynomials (CRC-32 and CRC-32C).  64 "lanes" run one after the other: aligned 16-byte granules,
// lane l taking granules l, l + 64, ...; the bytes of the first and last granule outside the chunk masked to 0; per round acc = acc x^8192 +
// g0 x^128 + g1 x^96 + g2 x^64 + g3 x^32; behind the chunk the multiply by x^(8 e) out of the 1 024-entry table and by x^-120; the fold as
// the kernel runs it (a run of chunks per lane, then the tree over the lanes).  EVERY LOAD IS CHECKED: a granule must hold a byte of the
// range, and it is read out of an allocation of exactly the range's end plus the 64 bytes of slack the ABI promises -- built with
// -fsanitize=address,undefined (tests/test_framing_compress_cpu.py), a load anywhere else ends the run.  Compared with a bit-by-bit CRC.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alz_checksum.h"

typedef uint32_t u32;
typedef uint64_t u64;

template <u32 P> static u32 bitwise(const uint8_t* p, size_t n) {
    u32 c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (P & (0u - (c & 1u))); }
    return c ^ 0xFFFFFFFFu;
}
static u32 byte_mask(int k) { return k <= 0 ? 0u : k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u; }

static long g_loads = 0;

// the raw CRC of the chunk [p, p + L) as the chunk kernel computes it; [lo, hi) is what may be read
template <u32 P> static u32 chunk_model(const uint8_t* p, u32 L, const uint8_t* lo, const uint8_t* hi) {
    static const alz_crc_xbyte_table<P> xbyte;
    const uintptr_t a0 = (uintptr_t)p & ~(uintptr_t)15;
    const u32 h = (u32)((uintptr_t)p - a0), span = h + L, Q = (span + 15u) >> 4;
    u32 all = 0;
    for (u32 lane = 0; lane < 64; lane++) {
        u32 acc = 0, q = lane;
        for (; q < Q; q += 64u) {
            const uint8_t* g = (const uint8_t*)(a0 + (uintptr_t)q * 16u);
            if (!(g + 16 > p && g < p + L)) { printf("granule %u holds no byte of the chunk\n", q); exit(2); }
            if (g < lo || g + 16 > hi) { printf("granule %u leaves the buffer and its slack\n", q); exit(2); }
            u32 d[4]; memcpy(d, g, 16); g_loads++;
            const int l0 = q == 0 ? (int)h : 0, h0 = (int)(span - q * 16u);
            if (l0 != 0 || h0 < 16) for (int w = 0; w < 4; w++) d[w] &= byte_mask(h0 - 4 * w) & ~byte_mask(l0 - 4 * w);
            acc = alz_crc_mul<P>(acc, alz_crc_xpow_c<P>(8192)) ^ alz_crc_mul<P>(d[0], alz_crc_xpow_c<P>(128)) ^ alz_crc_mul<P>(d[1], alz_crc_xpow_c<P>(96)) ^
                  alz_crc_mul<P>(d[2], alz_crc_xpow_c<P>(64)) ^ alz_crc_mul<P>(d[3], alz_crc_xpow_c<P>(32));
        }
        if (q != lane) {
            const int e = (int)span - (int)(16u * (q - 63u));
            if (e < -15 || e > 1008) { printf("e = %d\n", e); exit(2); }
            all ^= alz_crc_mul<P>(acc, xbyte.v[e + 15]);
        }
    }
    return alz_crc_mul<P>(all, alz_crc_xinv120<P>());
}

// the finished CRC of [p, p + len) from its chunks' raw CRCs, as the fold kernel joins them
template <u32 P, u32 KIND> static u32 range_model(const uint8_t* p, u32 len, u32 chunk, const uint8_t* lo, const uint8_t* hi) {
    const u32 C = (u32)(((u64)len + chunk - 1) / chunk);
    std::vector<u32> partial(C);
    for (u32 c = 0; c < C; c++) { const u64 off = (u64)c * chunk; partial[c] = chunk_model<P>(p + off, (u32)(len - off < chunk ? len - off : chunk), lo, hi); }
    const u32 m = (C + 63u) / 64u, xck = alz_crc_xpow_bytes<P>(chunk);
    u32 v[64], bytes[64];
    for (u32 lane = 0; lane < 64; lane++) {
        const u32 c0 = lane * m < C ? lane * m : C, c1 = c0 + m < C ? c0 + m : C;
        v[lane] = 0; bytes[lane] = 0;
        for (u32 c = c0; c < c1; c++) {
            const u64 left = (u64)len - (u64)c * chunk; const u32 cl = left < chunk ? (u32)left : chunk;
            v[lane] = alz_checksum_join(KIND, v[lane], partial[c], cl, cl == chunk ? xck : alz_crc_xpow_bytes<P>(cl));
            bytes[lane] += cl;
        }
    }
    const u32 used = m ? (C + m - 1u) / m : 0u;
    for (u32 o = 1; o < used; o <<= 1) {
        u32 nv[64], nb[64];
        for (u32 lane = 0; lane < 64; lane++) {
            const u32 from = lane + o < 64 ? lane + o : lane;                  // __shfl_down: a lane past the end reads itself
            const u32 pv = v[from], pb = bytes[from];
            const u32 j = alz_checksum_join(KIND, v[lane], pv, pb, alz_crc_xpow_bytes<P>(pb));
            nv[lane] = v[lane]; nb[lane] = bytes[lane];
            if ((lane & (2u * o - 1u)) == 0 && lane + o < 64u) { nv[lane] = j; nb[lane] = bytes[lane] + pb; }
        }
        memcpy(v, nv, sizeof(v)); memcpy(bytes, nb, sizeof(bytes));
    }
    return v[0] ^ alz_crc_mul<P>(0xFFFFFFFFu, alz_crc_xpow_bytes<P>(len)) ^ 0xFFFFFFFFu;
}

template <u32 P, u32 KIND> static long check(u32 off, u32 len, u32 chunk, u32 seed) {
    // the source buffer starts at a 16-byte boundary (device allocations do) and ends 64 readable bytes behind the range
    void* mem = nullptr;
    const size_t size = (size_t)off + len + 64;
    if (posix_memalign(&mem, 16, size)) { printf("no memory\n"); exit(2); }
    uint8_t* b = (uint8_t*)mem;
    u32 s = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < size; i++) { s = s * 1664525u + 1013904223u; b[i] = (uint8_t)(s >> 24); }
    const u32 got = range_model<P, KIND>(b + off, len, chunk, b, b + size), want = bitwise<P>(b + off, len);
    free(mem);
    if (got != want) { printf("P %08x off %u len %u: model %08x, bit by bit %08x\n", P, off, len, got, want); return 1; }
    return 0;
}

int main() {
    long bad = 0, cases = 0;
    const u32 chunk = ALZ_CHECKSUM_CHUNK;
    for (u32 len = 0; len <= 200; len++)
        for (u32 off = 0; off < 16; off++) { bad += check<ALZ_CRC32C_POLY, ALZ_CK_CRC32C>(off, len, chunk, len * 16 + off); bad += check<ALZ_CRC_POLY, ALZ_CK_CRC32>(off, len, chunk, len * 16 + off); cases += 2; }
    const u32 longs[] = {chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 1};
    for (u32 len : longs)
        for (u32 off : {0u, 1u, 15u}) { bad += check<ALZ_CRC32C_POLY, ALZ_CK_CRC32C>(off, len, chunk, len + off); bad += check<ALZ_CRC_POLY, ALZ_CK_CRC32>(off, len, chunk, len + off); cases += 2; }
    bad += check<ALZ_CRC32C_POLY, ALZ_CK_CRC32C>(13, 70 * 1024 + 5, 1024, 7); cases++;   // 71 chunks: more than one chunk per fold lane
    const uint8_t nine[] = "123456789";
    if (bitwise<ALZ_CRC32C_POLY>(nine, 9) != 0xE3069283u || bitwise<ALZ_CRC_POLY>(nine, 9) != 0xCBF43926u) { printf("check values\n"); bad++; }
    if (alz_checksum_join(ALZ_CK_CRC32C, 0x12345678u, 0, 0, alz_crc_xpow_bytes<ALZ_CRC32C_POLY>(0)) != 0x12345678u) { printf("join with nothing\n"); bad++; }
    printf("%ld cases, %ld loads, %ld bad\n", cases, g_loads, bad);
    return bad ? 1 : 0;
}
