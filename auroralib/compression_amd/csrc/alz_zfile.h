// alz_zfile.h -- the framing of RFC 1950 (zlib) and RFC 1952 (gzip) as zlib reads it: header walks, trailer fields and the host-side
// checksums.  Shared by the single-file layer (alz_inflate_file.cpp) and the batched one (alz_zfile.cpp), so that both judge a header and a
// trailer with the same code.  Pure host code; not part of the ABI.
#pragma once
#include <cstring>

#include "auroralz.h"

namespace alz_zframe {

const uint32_t kMaxCap = 0xFFFFFF00u;                                          // the largest dst_cap of a stream

inline uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = n < 5552 ? n : 5552;                                         // the longest run whose sums stay below 2^32
        n -= k;
        while (k--) { a += *p++; b += a; }
        a %= 65521u; b %= 65521u;
    }
    return (b << 16) | a;
}

struct Crc32 {
    uint32_t t[256];
    Crc32() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
    uint32_t of(const uint8_t* p, size_t n) const {
        uint32_t c = 0xFFFFFFFFu;
        while (n--) c = t[(c ^ *p++) & 0xFFu] ^ (c >> 8);
        return ~c;
    }
};
inline const Crc32& crc32() { static const Crc32 k; return k; }

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[3] | ((uint32_t)p[2] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[0] << 24); }

const size_t kZlibHeader = 2, kZlibTrailer = 4, kGzipTrailer = 8;

// RFC 1950: CMF, FLG in front of the body: ALZ_OK, ALZ_E_FORMAT or ALZ_E_UNSUPPORTED
inline int zlib_header(const uint8_t* src, size_t len) {
    if (len < 2) return ALZ_E_FORMAT;
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf & 0x0Fu) != 8u) return ALZ_E_FORMAT;                               // CM
    if ((cmf >> 4) > 7u) return ALZ_E_FORMAT;                                   // CINFO (it does not limit distances: inflate with 15 window bits)
    if ((cmf * 256u + flg) % 31u != 0u) return ALZ_E_FORMAT;                    // FCHECK
    if (flg & 0x20u) return ALZ_E_UNSUPPORTED;                                  // FDICT: no preset dictionaries
    return ALZ_OK;
}
// ... and behind it the big-endian Adler-32 of the output
inline bool zlib_trailer_ok(const uint8_t* trailer, uint32_t adler) { return be32(trailer) == adler; }

// the header of one gzip member at src[pos..len): ALZ_OK and pos behind it, ALZ_E_FORMAT, ALZ_E_CHECKSUM, or ALZ_E_STREAM (it runs past the input)
inline int gzip_header(const uint8_t* src, size_t len, size_t& pos) {
    const size_t start = pos, n = len - pos;
    if (n < 2 || src[pos] != 0x1F || src[pos + 1] != 0x8B) return ALZ_E_FORMAT;
    if (n >= 3 && src[pos + 2] != 8) return ALZ_E_FORMAT;                       // CM
    if (n >= 4 && (src[pos + 3] & 0xE0u)) return ALZ_E_FORMAT;                  // reserved FLG bits
    if (n < 10) return ALZ_E_STREAM;
    const uint32_t flg = src[pos + 3];
    pos += 10;                                                                  // MTIME, XFL, OS are not looked at
    if (flg & 4u) {                                                             // FEXTRA: XLEN, then XLEN bytes
        if (len - pos < 2) return ALZ_E_STREAM;
        const size_t xlen = (size_t)src[pos] | ((size_t)src[pos + 1] << 8);
        pos += 2;
        if (len - pos < xlen) return ALZ_E_STREAM;
        pos += xlen;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {                            // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        const void* z = memchr(src + pos, 0, len - pos);
        if (!z) return ALZ_E_STREAM;
        pos = (size_t)((const uint8_t*)z - src) + 1;
    }
    if (flg & 2u) {                                                             // FHCRC: the low 16 bits of the CRC-32 of the header so far
        if (len - pos < 2) return ALZ_E_STREAM;
        const uint32_t want = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
        if ((crc32().of(src + start, pos - start) & 0xFFFFu) != want) return ALZ_E_CHECKSUM;
        pos += 2;
    }
    return ALZ_OK;
}
// does another member start at src[pos..len)?  Anything else behind a member ends decoding
inline bool gzip_member_follows(const uint8_t* src, size_t len, size_t pos) { return len - pos >= 2 && src[pos] == 0x1F && src[pos + 1] == 0x8B; }
// the trailer of a member: the CRC-32 of its output (taken as correct without `crc`: a measure has no bytes) and ISIZE, its length
// (a stream holds fewer than 2^32 bytes: ISIZE is its length)
inline bool gzip_trailer_ok(const uint8_t* trailer, const uint32_t* crc, uint32_t member_len) {
    return (!crc || le32(trailer) == *crc) && le32(trailer + 4) == member_len;
}

}   // namespace alz_zframe
