// alz_framing.h -- the framing of LZ4 files (frame, legacy, skippable) and of framed Snappy files as the managed readers walk it, written once:
// alz_container.cpp (decode) and alz_container_measure.cpp (sizes) turn what these two pull parsers return into GPU work, each with its own
// scheduling.  Pure host code: no HIP, no call into the ABI, nothing allocated but the caller's block list -- so it runs on untrusted bytes under the
// sanitizers (tests/framing_walk_check.cpp).  Cited per function, paths relative to the reference's src.  Not part of the ABI.
// Behind the readers: the WRITERS' rules (frame descriptor, block words, end marks, Snappy chunk headers, the error mapping and the order
// in which a file is laid out and judged against its capacity), written once for alz_container.cpp (one file, pieces copied on the host)
// and alz_framing_compress.cpp (a batch, pieces copied in HBM).
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

// ---------------------------------------------------------------------------------------------- the writers
// A writer lays a file out as pieces in file order and hands each to a sink, which copies it (one file) or records it (a batch):
//   sink.bytes(at, p, k)       k <= 8 bytes the writer made up: magic, descriptor, size word, chunk header, end mark
//   sink.slot(at, i, k)        the first k bytes of block i's compressed output
//   sink.source(at, off, k)    k raw bytes of the input from `off`: a stored block or chunk
// `at` is the place in the file.  A writer that returns another code than ALZ_OK may have handed over pieces of the file in front of the
// failure: the bytes of a failed file are unspecified.
inline void wr_le32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// the BD byte of a frame for the block size a caller asks for (0: the default, 4 MiB), or 0 for a size the format does not have  LZ4.Frame.cs:29-35
inline uint8_t lz4_frame_bd(uint32_t option, uint32_t* block) {
    switch (option) {
    case 0: case 0x400000: *block = 0x400000; return 0x70;
    case 0x10000: *block = 0x10000; return 0x40;
    case 0x40000: *block = 0x40000; return 0x50;
    case 0x100000: *block = 0x100000; return 0x60;
    default: return 0;
    }
}
// magic, FLG, BD, HC.  `Flags &= IsVersion1` (LZ4.Frame.cs:184) leaves only the version bit: no content size, no checksums, blocks flagged linked
inline size_t lz4_frame_descriptor(uint8_t out[7], uint8_t bd) {
    wr_le32(out, kLz4Frame); out[4] = 0x40; out[5] = bd; out[6] = (uint8_t)((xxh32(out + 4, 2, 0) >> 8) & 0xFF);
    return 7;
}
inline uint32_t lz4_block_word(uint32_t len, bool stored) { return stored ? len | 0x80000000u : len; }
const uint32_t kLz4EndMark = 0;                                                          // a frame ends with a block word of 0
const uint8_t kLz4LegacyEof = 0xFF;                                                      // LZ4.cs:157
const uint32_t kLz4LegacyBlock = 0x800000u;                                              // (int)BlockMaxSizes.Block4MB * 2
const uint32_t kSnappyChunk = 0x10000u;                                                  // Snappy.cs:74
// a block the encoder did not finish: only LZ4 tells a slot that was too small apart
inline int lz4_block_error(int32_t status) { return status == ALZ_ST_OUTPUT_CAPACITY ? ALZ_E_NOMEM : ALZ_E_INVALID; }
inline int snappy_block_error(int32_t) { return ALZ_E_INVALID; }

inline uint32_t snappy_crc_mask(uint32_t crc) { return ((crc >> 15) | (crc << 17)) + 0xa282ead8u; }   // Snappy.cs:252
// type, u24 length (the CRC counts), the masked CRC-32C of the chunk's RAW bytes; `crc` is the plain CRC-32C
inline size_t snappy_chunk_header(uint8_t out[8], bool stored, uint32_t body, uint32_t crc) {
    const uint32_t len = body + 4;
    out[0] = stored ? 1 : 0; out[1] = (uint8_t)len; out[2] = (uint8_t)(len >> 8); out[3] = (uint8_t)(len >> 16);
    wr_le32(out + 4, snappy_crc_mask(crc));
    return 8;
}
// the slot of a block's compressed output in the encode batch of a writer
inline size_t write_slot_bytes(size_t block) { return (block + block / 4 + 64 + 255) & ~(size_t)255; }

// LZ4.Compress  LZ4.cs:113-160 (legacy) / CompressLZ4FrameHeader  LZ4.Frame.cs:176-229
struct Lz4Writer { bool legacy; uint32_t block; uint8_t bd; };
// what the writer refuses before it encodes anything; `option`: the frame's block size as the caller states it
inline int lz4_write_open(bool legacy, uint32_t option, size_t n, size_t cap, Lz4Writer& w) {
    w.legacy = legacy; w.block = kLz4LegacyBlock; w.bd = 0;
    if (cap < 16) return ALZ_E_NOMEM;
    if (!legacy && !(w.bd = lz4_frame_bd(option, &w.block))) return ALZ_E_INVALID;
    if (n && n % w.block != 0 && n % w.block < 5) return ALZ_E_INVALID;                  // source.Slice(0, Length - 5) throws  LZ4.cs:208
    return ALZ_OK;
}
// the file from the results `rs` of its blocks (block i: the bytes from i * w.block, at most w.block of them)
template <class Sink>
inline int lz4_write_blocks(const Lz4Writer& w, size_t n, const alz_result* rs, size_t cap, Sink& sink, size_t* file_len) {
    uint8_t h[8]; size_t o = 0;
    if (w.legacy) { wr_le32(h, kLz4Legacy); sink.bytes(0, h, 4); o = 4; }
    else { o = lz4_frame_descriptor(h, w.bd); sink.bytes(0, h, o); }
    const size_t nb = (n + w.block - 1) / w.block;
    for (size_t i = 0; i < nb; i++) {
        const size_t bl = n - i * w.block < w.block ? n - i * w.block : w.block;
        if (rs[i].status != ALZ_ST_OK) return lz4_block_error(rs[i].status);
        const bool stored = !w.legacy && rs[i].dst_len >= w.block;                       // buffer.Position >= (int)BlockSize: stored
        const size_t body = stored ? bl : rs[i].dst_len;
        if (o + 4 + body > cap) return ALZ_E_NOMEM;
        wr_le32(h, lz4_block_word((uint32_t)body, stored)); sink.bytes(o, h, 4);
        if (stored) sink.source(o + 4, i * (size_t)w.block, body); else sink.slot(o + 4, i, body);
        o += 4 + body;
    }
    if (w.legacy) { if (o + 1 > cap) return ALZ_E_NOMEM; h[0] = kLz4LegacyEof; sink.bytes(o, h, 1); o += 1; }
    else { if (o + 4 > cap) return ALZ_E_NOMEM; wr_le32(h, kLz4EndMark); sink.bytes(o, h, 4); o += 4; }
    *file_len = o;
    return ALZ_OK;
}

// Snappy.Compress  Formats/Common/Snappy.cs:71-107
inline int snappy_write_open(size_t cap) { return cap < 10 ? ALZ_E_NOMEM : ALZ_OK; }
// crc(i): the plain CRC-32C of the raw bytes of chunk i
template <class Sink, class Crc>
inline int snappy_write_chunks(size_t n, const alz_result* rs, size_t cap, Sink& sink, Crc crc, size_t* file_len) {
    sink.bytes(0, kSnappyId, 10);
    uint8_t h[8]; size_t o = 10;
    const size_t nb = (n + kSnappyChunk - 1) / kSnappyChunk;
    for (size_t i = 0; i < nb; i++) {
        const size_t cs = n - i * kSnappyChunk < kSnappyChunk ? n - i * kSnappyChunk : kSnappyChunk;
        if (rs[i].status != ALZ_ST_OK) return snappy_block_error(rs[i].status);
        const bool stored = rs[i].dst_len >= cs;                                         // buffer.Length >= chunkSize
        const size_t body = stored ? cs : rs[i].dst_len;
        snappy_chunk_header(h, stored, (uint32_t)body, crc(i));
        if (o + 8 + body > cap) return ALZ_E_NOMEM;
        sink.bytes(o, h, 8);
        if (stored) sink.source(o + 8, i * (size_t)kSnappyChunk, body); else sink.slot(o + 8, i, body);
        o += 8 + body;
    }
    *file_len = o;
    return ALZ_OK;
}

}  // namespace alz_framing
