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

// ZLib.IsMatchStatic  ZLib.cs:26-27: Position + 4 < Length && CheckZlibHeaderAndFirstBlock(Peek<uint>())  :52-76
inline bool zlib_is_match(const uint8_t* src, size_t src_len) {
    if (!src || !(src_len > 4)) return false;
    const uint32_t cmf = src[0], flg = src[1], d1 = src[2], d2 = src[3];
    if ((cmf & 0x0Fu) != 8u) return false;                                      // CM != deflate
    if (((cmf >> 4) & 0x0Fu) > 7u) return false;                                // CINFO > 7
    if ((cmf * 256u + flg) % 31u != 0u) return false;
    const uint32_t btype = (d1 >> 1) & 3u;
    if (btype == 3u) return false;
    if (btype == 0u) {                                                          // as written: LEN is read from the first two data bytes  :70
        const uint16_t len = (uint16_t)(d1 | (d2 << 8)), nlen = (uint16_t)~len;
        if ((len ^ nlen) != 0xFFFF) return false;
        if (len == 0) return false;
    }
    return true;
}

}   // namespace alz_zframe

// The walks of the wrapped files (alz_wfile_*, alz_wfile.cpp): the eight classes of the reference that are a small header over a body the
// library already decodes.  Pure host code: every read is checked against `len` first.  Paths are relative to the reference's
// src/AuroraLib.Compression-Extended, RLHudson's to src/AuroraLib.Compression.Nintendo.
namespace alz_wframe {

using alz_zframe::be32;
using alz_zframe::le32;
inline uint32_t rd32(const uint8_t* p, bool big) { return big ? be32(p) : le32(p); }
inline uint32_t swap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// the 12-byte header of a WFLZ file behind its magic (WFLZ.cs:50-60): compressed size and size in FormatByteOrder.  The caller has
// checked the magic and that 12 bytes are there.  The compressed span is what the file still holds of it (Stream.Read returns what is there).
inline void wflz_header(const uint8_t* src, size_t len, bool big, uint32_t* csz, uint32_t* size) {
    const uint32_t c = rd32(src + 4, big);
    const size_t left = len - 12;
    *csz = c > left ? (uint32_t)(left > 0xFFFFFFFFu ? 0xFFFFFFFFu : left) : c;
    *size = rd32(src + 8, big);
}

// SSZL's keystream: the MersenneTwister variant of Specialized/SSZL.cs:200-282, restated exactly -- 31-bit state words, the initialisation by
// (i + 1) - 0x13F8769B * (cur ^ cur >> 30), a twist per draw, and the ARITHMETIC shift in Temper.
const uint32_t kSszlSeed = 0x40C360F3u;
struct SszlTwister {
    uint32_t buf[624]; int index;
    explicit SszlTwister(uint32_t seed = kSszlSeed) {
        buf[0] = seed & 0x7FFFFFFFu; index = 624;                               // :223-224
        for (int i = 0; i < 623; i++) {                                         // :226-233
            const uint32_t cur = buf[i], tmp = cur ^ (cur >> 30), mul = 0x13F8769Bu * tmp;
            buf[i + 1] = ((uint32_t)(i + 1) - mul) & 0x7FFFFFFFu;
        }
    }
    uint32_t next() {                                                           // :239-262
        if (index == 624) index = 0;
        const uint32_t a = buf[index], b = buf[(index + 1) % 624], c = buf[(index + 397) % 624];
        const uint32_t part = (a ^ ((a ^ b) & 0x7FFFFFFFu)) >> 1;               // Twist  :264-268
        const uint32_t v = (part ^ c ^ (0x1908B0DFu * (b & 1u))) & 0x7FFFFFFFu;
        buf[index++] = v;
        const uint32_t t1 = (v >> 11) ^ v, t3 = ((t1 & 0xFF3A58ADu) << 7) ^ t1, t5 = ((t3 & 0xFFFFDF8Cu) << 15) ^ t3;   // Temper  :270-282
        const int32_t s = (int32_t)t5;
        return (uint32_t)(s ^ (s >> 18)) & 0x7FFFFFFFu;                         // (int)t5 >> 18: arithmetic
    }
};
// MTXorTransform (:169-195) over a keystream drawn before: whole little-endian words, then 1-3 bytes of one more word
inline void sszl_xor(uint8_t* p, size_t n, const uint32_t* ks) {
    for (size_t i = 0; i < n; i++) p[i] ^= (uint8_t)(ks[i >> 2] >> (8 * (i & 3)));
}

// ALZ_OK: the `n` bytes of `m` are there; ALZ_E_FORMAT: other bytes; ALZ_E_STREAM: the file ends inside them and agrees so far
inline int magic(const uint8_t* src, size_t len, const void* m, size_t n) {
    if (memcmp(src, m, len < n ? len : n)) return ALZ_E_FORMAT;
    return len < n ? ALZ_E_STREAM : ALZ_OK;
}

// HWGZ's Header.TryRead (Specialized/HWGZ.cs:149-164): little endian first, then big; false: neither validates
struct HwgzHeader { uint32_t chunk_size, count, size; };
inline bool hwgz_validate(const HwgzHeader& h) { return h.count != 0 && h.count == (uint32_t)(h.size + h.chunk_size - 1u) / h.chunk_size; }   // :140 (uint arithmetic)
inline bool hwgz_header(const uint8_t* src, HwgzHeader* h) {
    h->chunk_size = le32(src); h->count = le32(src + 4); h->size = le32(src + 8);
    if (h->chunk_size == 0 || h->count == 0 || h->size == 0) return false;      // :153-154
    if (hwgz_validate(*h)) return true;
    h->chunk_size = swap32(h->chunk_size); h->count = swap32(h->count); h->size = swap32(h->size);
    return h->chunk_size != 0 && hwgz_validate(*h);                             // (a reversed word of a non-zero word is non-zero)
}

// IsMatchStatic of each class, statement for statement
inline int is_match(uint32_t kind, const uint8_t* src, size_t len) {
    if (!src) return 0;
    switch (kind) {
    case ALZ_WF_ASURAZLB: return len > 0x14 && !memcmp(src, "AsuraZlb", 8);     // EA/AsuraZlb.cs:33
    case ALZ_WF_ZLB:      return len > 0x14 && !memcmp(src, "ZLB\0", 4);        // Rare/ZLB.cs:35 (0x14 behind a 16-byte header)
    case ALZ_WF_MDF0:     return len > 0x10 && !memcmp(src, "mdf\0", 4) && le32(src + 4) != 0 && alz_zframe::zlib_is_match(src + 8, len - 8);   // Konami/MDF0.cs:32
    case ALZ_WF_RAREZIP:  return len > 6 && src[0] == 0x11 && src[1] == 0x72 && be32(src + 2) != 0;   // Rare/RareZip.cs:29
    case ALZ_WF_HWGZ: {                                                         // Specialized/HWGZ.cs:36-49
        if (len < 0x80) return 0;
        HwgzHeader h;
        if (!hwgz_header(src, &h)) return 0;
        const uint64_t pos = align_up(12 + 4ull * h.count, 128) + 4;            // Align(4 * count, Current, 128), then At(4, Current)
        return pos < len && alz_zframe::zlib_is_match(src + pos, len - (size_t)pos);
    }
    case ALZ_WF_SSZL:     return len > 0x10 && !memcmp(src, "SSZL", 4) && le32(src + 4) == 0x20101109u;   // Specialized/SSZL.cs:73
    case ALZ_WF_ZLWF:     return len > 0x10 && !memcmp(src, "ZLWF", 4);         // WayForward/ZLWF.cs:40
    case ALZ_WF_RLHUDSON: return len > 6 && len >= 8 && be32(src) != 0 && be32(src + 4) == 5;   // HudsonSoft/RLHudson.cs:30 (7 bytes: the second ReadInt32 throws)
    default: return 0;
    }
}

// the walk of one file: its parts, the size its header states and (SSZL) its Options.  ALZ_OK; ALZ_E_FORMAT: wrong magic or an invalid HWGZ
// header; ALZ_E_STREAM: a header, a table or a chunk runs past the input (INPUT_TRUNCATED); ALZ_E_INVALID: unknown kind, or `cap` parts do
// not hold the file's (then *n_parts is the count needed).  parts may be NULL with cap 0.
inline int walk(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, alz_wfile_part* parts, uint32_t cap,
                uint32_t* n_parts, uint32_t* stated, uint32_t* flags) {
    const bool big = opt && opt->big_endian;
    uint32_t n = 0, size = 0, fl = 0;
    int rc = ALZ_OK;
    auto put = [&](uint64_t off, uint64_t plen, uint32_t body, uint32_t dlen) {
        if (n < cap && parts) { parts[n].src_off = (uint32_t)off; parts[n].src_len = (uint32_t)plen; parts[n].body = body; parts[n].dst_len = dlen; }
        n++;
    };
    auto bounded = [&](size_t hdr, uint32_t csize) { const size_t left = len - hdr; put(hdr, csize < left ? csize : left, ALZ_WB_ZLIB, 0); };
    if (n_parts) *n_parts = 0;
    if (stated) *stated = 0;
    if (flags) *flags = 0;
    if ((len && !src) || len > 0xFFFFFF00u) return ALZ_E_INVALID;
    switch (kind) {
    case ALZ_WF_ASURAZLB:                                                       // AsuraZlb.cs:45-65
        if ((rc = magic(src, len, "AsuraZlb", 8))) return rc;
        if (len < 20) return ALZ_E_STREAM;
        size = be32(src + 16); bounded(20, be32(src + 12));
        break;
    case ALZ_WF_ZLB:                                                            // ZLB.cs:46-70
        if ((rc = magic(src, len, "ZLB\0", 4))) return rc;
        if (len < 16) return ALZ_E_STREAM;
        size = be32(src + 8); bounded(16, be32(src + 12));
        break;
    case ALZ_WF_MDF0:                                                           // MDF0.cs:43-54
        if ((rc = magic(src, len, "mdf\0", 4))) return rc;
        if (len < 8) return ALZ_E_STREAM;
        size = le32(src + 4); put(8, len - 8, ALZ_WB_ZLIB, 0);
        break;
    case ALZ_WF_RAREZIP:                                                        // RareZip.cs:40-54
        if ((rc = magic(src, len, "\x11\x72", 2))) return rc;
        if (len < 6) return ALZ_E_STREAM;
        size = be32(src + 2); put(6, len - 6, ALZ_WB_DEFLATE, 0);
        break;
    case ALZ_WF_HWGZ: {                                                         // HWGZ.cs:61-83
        if (len < 12) return ALZ_E_STREAM;
        HwgzHeader h;
        if (!hwgz_header(src, &h)) return ALZ_E_FORMAT;
        size = h.size;
        if (12 + 4ull * h.count > len) return ALZ_E_STREAM;                     // more chunks than the file can hold
        uint64_t pos = align_up(12 + 4ull * h.count, 128);
        for (uint32_t i = 0; i < h.count; i++) {
            if (pos + 4 > len) { rc = ALZ_E_STREAM; break; }
            const uint32_t csize = rd32(src + pos, big);                        // FormatByteOrder, whatever the header's order was  :76
            if (csize > len - (pos + 4)) { rc = ALZ_E_STREAM; break; }          // a chunk outside the file
            put(pos + 4, csize, ALZ_WB_ZLIB, 0);
            pos = align_up(pos + 4 + csize, 128);                               // Align(128)  :78
        }
        if (rc) { if (n_parts) *n_parts = 0; if (stated) *stated = size; return rc; }
        break;
    }
    case ALZ_WF_SSZL: {                                                         // SSZL.cs:85-118
        if ((rc = magic(src, len, "SSZL", 4))) return rc;
        if (len < 20) return ALZ_E_STREAM;
        size = le32(src + 8); fl = le32(src + 12);
        if (!(fl & 1u)) { put(20, len - 20, ALZ_WB_PLAIN, 0); break; }          // not Compressed: the bytes are copied
        if (len - 20 < 2) { if (flags) *flags = fl; if (stated) *stated = size; return ALZ_E_STREAM; }   // Peek<ushort> throws
        uint32_t two = (uint32_t)src[20] | ((uint32_t)src[21] << 8);
        if (fl & 0x80000000u) { SszlTwister mt; two = (two ^ mt.next()) & 0xFFFFu; }
        put(20, len - 20, two == 0x8B1Fu ? ALZ_WB_GZIP : ALZ_WB_ZLIB, 0);
        break;
    }
    case ALZ_WF_ZLWF: {                                                         // ZLWF.cs:53-95
        if ((rc = magic(src, len, "ZLWF", 4))) return rc;
        if (len < 16) return ALZ_E_STREAM;
        size = rd32(src + 8, big);
        const uint32_t chunks = rd32(src + 12, big);
        if (16 + 4ull * chunks > len) { if (stated) *stated = size; return ALZ_E_STREAM; }
        for (uint32_t i = 0; i < chunks && !rc; i++) {
            const uint64_t off = rd32(src + 16 + 4 * (size_t)i, big);           // every entry swapped, as the NET8 branch does
            if (off + 12 > len) { rc = ALZ_E_STREAM; break; }
            if (memcmp(src + off, "WFLZ", 4)) { rc = ALZ_E_FORMAT; break; }
            uint32_t csz, dsz;
            wflz_header(src + off, len - (size_t)off, big, &csz, &dsz);
            put(off + 12, csz, big ? ALZ_WB_WFLZ_BE : ALZ_WB_WFLZ, dsz);
        }
        if (rc) { if (stated) *stated = size; return rc; }
        break;
    }
    case ALZ_WF_RLHUDSON:                                                       // RLHudson.cs:37-43 (the identifier is read and not compared)
        if (len < 8) return ALZ_E_STREAM;
        size = be32(src); put(8, len - 8, ALZ_WB_RLHUDSON, size);
        break;
    default: return ALZ_E_INVALID;
    }
    if (n_parts) *n_parts = n;
    if (stated) *stated = size;
    if (flags) *flags = fl;
    return n > cap ? ALZ_E_INVALID : ALZ_OK;
}

// GetDecompressedSize of each class
inline int decompressed_size(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, uint32_t* size_out) {
    uint32_t n = 0, fl = 0;
    if (!size_out) return ALZ_E_INVALID;
    if (kind == ALZ_WF_HWGZ || kind == ALZ_WF_ZLWF || kind == ALZ_WF_SSZL) {    // (the header alone: chunks and payload are not looked at)
        if ((len && !src)) return ALZ_E_INVALID;
        if (kind == ALZ_WF_HWGZ) {
            HwgzHeader h;
            if (len < 12) return ALZ_E_STREAM;
            if (!hwgz_header(src, &h)) return ALZ_E_FORMAT;
            *size_out = h.size; return ALZ_OK;
        }
        if (int rc = magic(src, len, kind == ALZ_WF_ZLWF ? "ZLWF" : "SSZL", 4)) return rc;
        if (len < 12) return ALZ_E_STREAM;
        *size_out = kind == ALZ_WF_ZLWF ? rd32(src + 8, opt && opt->big_endian) : le32(src + 8);
        return ALZ_OK;
    }
    const int rc = walk(kind, opt, src, len, nullptr, 0, &n, size_out, &fl);
    return rc == ALZ_E_INVALID && n ? ALZ_OK : rc;                              // (no room for parts was asked for)
}

}   // namespace alz_wframe
