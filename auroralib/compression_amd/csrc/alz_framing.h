// alz_framing.h -- the framing of LZ4 files (frame, legacy, skippable) and of framed Snappy files as the managed readers walk it, written once:
// alz_container.cpp (decode) and alz_container_measure.cpp (sizes) turn what these two pull parsers return into GPU work, each with its own
// scheduling.  Pure host code: no HIP, no call into the ABI, nothing allocated but the caller's block list -- so it runs on untrusted bytes under the
// sanitizers (tests/framing_walk_check.cpp).  Cited per function, paths relative to the reference's src.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "auroralz.h"

namespace alz_framing {

inline uint32_t le32(const uint8_t* p) { return ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0]; }
inline uint32_t le24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
inline uint32_t clamp32(size_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// XXH32 (the LZ4 frame format's checksum; the reference takes it as LZ4.HashAlgorithm, LZ4.Frame.cs:17-18)
inline uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
inline uint32_t xxh32(const uint8_t* p, size_t len, uint32_t seed) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    const uint8_t* end = p + len; uint32_t h;
    if (len >= 16) {
        uint32_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        do {
            v1 = rotl32(v1 + le32(p) * P2, 13) * P1; v2 = rotl32(v2 + le32(p + 4) * P2, 13) * P1;
            v3 = rotl32(v3 + le32(p + 8) * P2, 13) * P1; v4 = rotl32(v4 + le32(p + 12) * P2, 13) * P1; p += 16;
        } while (p + 16 <= end);
        h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
    } else h = seed + P5;
    h += (uint32_t)len;
    while (p + 4 <= end) { h = rotl32(h + le32(p) * P3, 17) * P4; p += 4; }
    while (p < end) { h = rotl32(h + (*p) * P5, 11) * P1; p++; }
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// ---------------------------------------------------------------------------------------------- LZ4: one frame per call
const uint32_t kLz4Legacy = 0x184C2102u, kLz4Frame = 0x184D2204u, kLz4SkippableFirst = 0x184D2A50u, kLz4SkippableLast = 0x184D2A5Fu;   // LZ4.Frame.cs:50-70
inline bool lz4_magic_skippable(uint32_t v) { return v >= kLz4SkippableFirst && v <= kLz4SkippableLast; }
inline bool lz4_magic_defined(uint32_t v) { return v == kLz4Legacy || v == kLz4Frame || lz4_magic_skippable(v); }

struct Lz4Block { size_t off; uint32_t len; bool raw; };

// What stands at one place of an LZ4 file.  The verdicts apply in this order, whoever reads them: the blocks run in file order and the first
// body that fails decides; only behind blocks that were all fine does `fault` decide, then `truncated` (the two exclude each other: the read
// stops at the first); then the declared content size, then the content checksum word at `end` (FLG bit 2), which is left to the caller -- a
// decoder verifies it, a size query skips it.
struct Lz4Frame {
    enum Kind { NOT_A_FRAME, LEGACY, FRAME, SKIPPABLE } kind;
    uint32_t flg, nominal;            // FLG of a frame; nominal: what a block holds and decodes to at most (the block maximum of a frame, 0x800000 legacy)
    uint64_t content;                 // the declared content size (FLG bit 3)
    size_t first, count;              // `blocks`: the blocks read completely (a checksummed block: verified), in file order, appended to the caller's list at `first`
    bool truncated;                   // the input ended inside the magic, the header or behind `blocks`
    int fault;                        // ALZ_OK, or what was met behind `blocks`: E_FORMAT (BD, a block above bmax), E_UNSUPPORTED (a dictionary), E_CHECKSUM (a block's)
    uint32_t next_magic;              // legacy: the defined magic that was read where a block size was expected (the next call's `magic`), else 0
    bool ends_file;                   // Decompress returns behind this: an undefined magic (end: in front of it), a legacy file that does not chain
    size_t end;                       // where the read stopped
    size_t behind(const Lz4Block& b) const { return b.off + b.len + (flg & 16 ? 4 : 0); }   // the position behind a block and its checksum word
};

// Reads what stands at `pos`: LZ4.Decompress  Formats/Common/LZ4.cs:50-93, ReadLZ4L :96-111, DecompressLZ4FrameHeader  LZ4.Frame.cs:107-174.
// magic = 0: the magic is read from the file; otherwise it is the previous legacy frame's next_magic and `pos` is behind it.  The blocks are appended
// to `blocks`, one list for as many frames as the caller keeps: what a file costs in memory stays linear in its size however many frames it has.
inline void lz4_read_frame(const uint8_t* src, size_t len, size_t pos, uint32_t magic, Lz4Frame& f, std::vector<Lz4Block>& blocks) {
    f.kind = Lz4Frame::NOT_A_FRAME; f.flg = f.nominal = 0; f.content = 0; f.first = blocks.size(); f.count = 0;
    f.truncated = false; f.fault = ALZ_OK; f.next_magic = 0; f.ends_file = false; f.end = pos;
    size_t& p = f.end;
    if (magic == 0) {
        if (p + 4 > len) { f.truncated = true; return; }
        magic = le32(src + p); p += 4;
    }
    if (magic == kLz4Legacy) {                                                           // LZ4.cs:96-111
        f.kind = Lz4Frame::LEGACY; f.nominal = 0x800000u;
        if (p + 4 > len) { f.truncated = true; return; }
        uint32_t bs = le32(src + p); p += 4;
        for (;;) {
            if (bs > len - p) { f.truncated = true; return; }
            blocks.push_back(Lz4Block{ p, bs, false }); f.count++; p += bs;
            if (p >= len) break;                                                         // ReadByte() == -1
            if (src[p] == 0xFF) { p++; break; }                                          // (sbyte)0xFF == -1: the EOF flag
            if (p + 4 > len) { f.truncated = true; return; }
            bs = le32(src + p); p += 4;
            if (lz4_magic_defined(bs)) { f.next_magic = bs; return; }
        }
        f.ends_file = true;                                                              // blockSize == 0: Decompress returns
    } else if (magic == kLz4Frame) {                                                     // LZ4.Frame.cs:107-174
        f.kind = Lz4Frame::FRAME;
        if (p + 2 > len) { f.truncated = true; return; }
        const uint32_t flg = f.flg = src[p], bd = src[p + 1]; p += 2;
        uint32_t bmax;
        switch ((bd & 0x70) >> 4) { case 4: bmax = 0x10000; break; case 5: bmax = 0x40000; break; case 6: bmax = 0x100000; break; case 7: bmax = 0x400000; break; default: f.fault = ALZ_E_FORMAT; return; }
        f.nominal = bmax;
        if (flg & 8) { if (p + 8 > len) { f.truncated = true; return; } f.content = (uint64_t)le32(src + p) | ((uint64_t)le32(src + p + 4) << 32); p += 8; }
        if (flg & 1) { if (p + 4 > len) { f.truncated = true; return; } p += 4; }
        if (p + 1 > len) { f.truncated = true; return; }
        p += 1;                                                                          // HeaderChecksum: read, not verified
        if (flg & 1) { f.fault = ALZ_E_UNSUPPORTED; return; }                            // external dictionaries  LZ4.Frame.cs:113-114
        // A block too large for the frame or with a wrong checksum ends the read; it decides the outcome only if the blocks in front of it
        // decode cleanly (the managed reader meets it after them).
        for (;;) {
            if (p + 4 > len) { f.truncated = true; return; }
            const uint32_t bsz = le32(src + p); p += 4;
            if (bsz == 0) return;                                                        // EndMark
            const bool raw = (bsz & 0x80000000u) != 0; const uint32_t n = bsz & 0x7FFFFFFFu;
            if (n > bmax) { f.fault = ALZ_E_FORMAT; return; }
            if (n > len - p) { f.truncated = true; return; }
            const size_t boff = p; p += n;
            if (flg & 16) {                                                              // block checksum over the stored bytes
                if (p + 4 > len) { f.truncated = true; return; }
                if (le32(src + p) != xxh32(src + boff, n, 0)) { f.fault = ALZ_E_CHECKSUM; return; }
                p += 4;
            }
            if (blocks.empty()) blocks.reserve(std::min<size_t>((len - boff) / (p - boff + 4) + 1, 1u << 16));   // (once per list, 1 MiB at most: were all blocks like the first -- 20 000 one-byte blocks otherwise grow it 15 times)
            blocks.push_back(Lz4Block{ boff, n, raw }); f.count++;
        }
    } else if (lz4_magic_skippable(magic)) {
        f.kind = Lz4Frame::SKIPPABLE;
        if (p + 4 > len) { f.truncated = true; return; }
        const uint32_t n = le32(src + p); p += 4;
        p = (uint64_t)p + n > len ? len : p + n;
    } else { p -= 4; f.ends_file = true; }                                               // not a frame: stop in front of it
}

// Does any match of this LZ4 block point in front of the block's own output?  (A walk over the sequences: input only.)  Offset 0 is a
// distance of 65 536 (E1): it reaches back while the block has produced less than that.
inline bool lz4_block_reaches_back(const uint8_t* b, uint32_t n) {
    uint64_t produced = 0; uint32_t p = 0;
    while (p < n) {
        const uint32_t tok = b[p++];
        uint64_t lit = tok >> 4;
        if (lit == 15) { uint32_t x; do { if (p >= n) return false; x = b[p++]; lit += x; } while (x == 255); }
        if (lit > n - p) return false;                                  // truncated: the decoder reports it
        p += (uint32_t)lit; produced += lit;
        if (p >= n) break;
        if (p + 2 > n) return false;
        const uint32_t dist = b[p] | (b[p + 1] << 8); p += 2;
        uint64_t ml = tok & 15;
        if (ml == 15) { uint32_t x; do { if (p >= n) return false; x = b[p++]; ml += x; } while (x == 255); }
        if ((dist == 0 ? 65536u : dist) > produced) return true;
        produced += ml + 4;
    }
    return false;
}

// ---------------------------------------------------------------------------------------------- framed Snappy: one chunk header per call
const uint8_t kSnappyId[10] = { 0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59 };                // Snappy.cs:17

inline uint32_t snappy_varint(const uint8_t* p, size_t len, size_t* used) {            // Snappy.ReadDecompressedSize  Snappy.cs:109-122
    uint32_t v = 0; int shift = 0; size_t i = 0; int b = 0x80;
    while ((b & 0x80) && i < len) { b = p[i++]; if (shift < 32) v |= (uint32_t)(b & 0x7F) << shift; shift += 7; }
    if (used) *used = i;
    return v;
}

struct SnappyChunk {
    enum Kind { COMPRESSED, STORED, SKIPPED, RESERVED, TRUNCATED } kind;
    size_t hdr, body;                 // the chunk header; the body: behind the CRC (COMPRESSED, STORED; CRCs are skipped as in the reference) or the header (SKIPPED)
    uint32_t len;                     // the declared length (the CRC counts)
    uint32_t stored;                  // STORED: the bytes of the body that the file holds (SubStream.CopyTo copies what is there)
    size_t next;                      // where the declared length leads, clipped to the file; RESERVED, TRUNCATED: where the read stopped (= body)
};

// The chunk header at `pos` < len: Snappy.Decompress  Formats/Common/Snappy.cs:39-69.  TRUNCATED: the input ends inside the header or the CRC,
// or a stored chunk is shorter than its CRC; RESERVED: an unskippable chunk type 0x02..0x7F (Snappy.cs:61-62).
inline SnappyChunk snappy_read_chunk(const uint8_t* src, size_t len, size_t pos) {
    SnappyChunk c = { SnappyChunk::TRUNCATED, pos, pos, 0, 0, pos };
    if (pos + 4 > len) return c;
    const uint32_t type = src[pos]; c.len = le24(src + pos + 1);
    c.body = c.next = pos + 4;
    if (type <= 1) {
        if (c.body + 4 > len || (type == 1 && c.len < 4)) return c;
        c.body += 4;
        c.kind = type == 0 ? SnappyChunk::COMPRESSED : SnappyChunk::STORED;
        if (type == 1) c.stored = c.len - 4 > len - c.body ? (uint32_t)(len - c.body) : c.len - 4;
    } else if (type <= 0x7F) { c.kind = SnappyChunk::RESERVED; return c; }
    else c.kind = SnappyChunk::SKIPPED;
    c.next = (uint64_t)pos + 4 + c.len > len ? len : pos + 4 + c.len;
    return c;
}

}  // namespace alz_framing
