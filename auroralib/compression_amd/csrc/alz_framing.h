// alz_framing.h -- the framing of LZ4 files (frame, legacy, skippable) and of framed Snappy files as the managed readers walk it, written once:
// alz_container.cpp (decode) and alz_container_measure.cpp (sizes) turn what these two pull parsers return into GPU work, each with its own
// scheduling.  Pure host code: no HIP, no call into the ABI, nothing allocated but the caller's block list -- so it runs on untrusted bytes under the
// sanitizers (tests/framing_walk_check.cpp).  Cited per function, paths relative to the reference's src.  Not part of the ABI.
// Behind the readers: what their records and the results of the bodies make of a file (rc, status, length, how far it was read), written once
// for the single-file measure and Snappy decode and for the batched measure and decode of alz_framed_batch.cpp (tests/framing_replay_check.cpp).
// Behind those: the WRITERS' rules (frame descriptor, block words, end marks, Snappy chunk headers, the error mapping and the order
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

inline bool snappy_has_id(const uint8_t* src, size_t len) { return len >= 10 && std::equal(kSnappyId, kSnappyId + 10, src); }

// ---------------------------------------------------------------------------------------------- from records and results to a file's outcome
// What the readers' records and the results of the bodies make of a file -- rc, status, length, how far it was read -- written once for the
// four layers that read such files: the single-file measure (alz_container_measure.cpp) and Snappy decode (alz_container.cpp), the batch
// measure and the batch decode (alz_framed_batch.cpp).  Those keep how bodies reach the GPU and how bytes move; a layer that moves bytes
// hands in a sink or a visitor.  tests/framing_replay_check.cpp runs these functions on results from the CPU oracle.
const uint32_t kNoBound = 0xFFFFFF00u;                                                   // the largest dst_cap of a stream
inline alz_stream body(uint32_t fmt, uint64_t src_off, size_t src_len, uint64_t dst_off, uint32_t dst_cap, uint32_t hist) {
    alz_stream s = {};
    s.src_off = src_off; s.src_len = clamp32(src_len); s.dst_off = dst_off; s.dst_cap = dst_cap; s.aux0 = hist; s.format = fmt;
    return s;
}
// A body measured with no bound on its count (dst_cap = kNoBound) tells what it does in ANY destination: with `room` bytes left it ends as
// measured when its bytes fit, and in OUTPUT_CAPACITY with the room used up otherwise (the first token that does not fit stops the decoder,
// in front of any later error).  Advances `out` by what the body leaves in a destination of `cap` bytes; returns its status there.
inline int32_t place_body(const alz_result& m, uint64_t& out, uint64_t cap) {
    const uint64_t room = out < cap ? cap - out : 0;
    if (m.dst_len > room) { out += room; return ALZ_ST_OUTPUT_CAPACITY; }
    out += m.dst_len;
    return m.status;
}

// rc is ALZ_OK, ALZ_E_STREAM (then `status` tells why) or the code that refuses the file; out: bytes delivered; pos: how far the file was read
struct Outcome { int rc; int32_t status; uint64_t out; size_t pos; };
inline Outcome stream_outcome(int32_t status, uint64_t out, size_t pos) { return Outcome{ status == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM, status, out, pos }; }
inline Outcome refused(int rc) { return Outcome{ rc, ALZ_ST_OK, 0, 0 }; }

// ---- LZ4
struct Lz4File { std::vector<Lz4Frame> frames; std::vector<Lz4Block> blocks; };

// LZ4.Decompress  Formats/Common/LZ4.cs:50-93: the frames of the file (where a block lies does not depend on what any block decodes to).
// measure(b): every compressed block, in file order -- the caller appends the body it is measured as.
template <class Measure>
inline void lz4_collect(const uint8_t* src, size_t len, Lz4File& w, Measure measure) {
    size_t pos = 0; uint32_t magic = 0;
    while (magic != 0 || pos < len) {
        w.frames.emplace_back(); Lz4Frame& f = w.frames.back();
        lz4_read_frame(src, len, pos, magic, f, w.blocks);
        pos = f.end; magic = f.next_magic;
        for (const Lz4Block* b = w.blocks.data() + f.first, *e = b + f.count; b != e; b++) if (!b->raw) measure(*b);
        if (f.fault != ALZ_OK || f.truncated || f.ends_file) break;
        if (f.flg & 4) { if (pos + 4 > len) break; pos += 4; }                           // content checksum: needs the bytes
    }
}

// What a size query hands to lz4_replay.  A decoder's visitor does its work in the same three places:
struct Lz4Sizes {
    // every block in file order with the output in front of it, the room behind that and (compressed blocks) its measured result; another
    // code than ALZ_OK refuses the file
    int block(const Lz4Frame&, const Lz4Block&, uint64_t /*frame_start*/, uint64_t /*out*/, uint64_t /*room*/, const alz_result*) { return ALZ_OK; }
    // a block ended the file short: where the read stands (a decoder has read the whole frame by then)
    size_t stopped(const Lz4Frame& f, const Lz4Block& b) { return f.behind(b); }
    // a frame that ended well carries a content checksum word at `pos` over out - frame_start bytes: taken as correct here
    void content_checksum(uint64_t /*frame_start*/, uint64_t /*out*/, size_t /*pos*/) {}
};

// The in-order reader over the measured sizes `m` (one per compressed block, file order; blocks of a linked frame are measured like
// independent ones: history only supplies bytes, never sizes).  The verdicts in the order Lz4Frame states: blocks in file order, then what
// the frame's read met behind them.
template <class Visitor>
inline Outcome lz4_replay(const Lz4File& w, size_t len, uint64_t cap, const alz_result* m, Visitor& v) {
    uint64_t out = 0; size_t pos = 0;
    for (const Lz4Frame& f : w.frames) {
        const uint64_t frame_start = out;
        for (const Lz4Block* b = w.blocks.data() + f.first, *e = b + f.count; b != e; b++) {
            const uint64_t room = cap - out;
            const alz_result* mb = b->raw ? nullptr : m++;
            if (const int rc = v.block(f, *b, frame_start, out, room, mb)) return refused(rc);
            int32_t st = ALZ_ST_OK;
            if (mb) st = place_body(*mb, out, cap);
            else if (b->len > room) { out += room; st = ALZ_ST_OUTPUT_CAPACITY; }        // what fits, as the window writes it
            else out += b->len;
            if (st != ALZ_ST_OK) return stream_outcome(st, out, v.stopped(f, *b));
        }
        pos = f.end;
        if (f.fault != ALZ_OK) return Outcome{ f.fault, ALZ_ST_OK, out, pos };
        if (f.truncated) return stream_outcome(ALZ_ST_INPUT_TRUNCATED, out, pos);
        if ((f.flg & 8) && out - frame_start != f.content) return stream_outcome(ALZ_ST_OUTPUT_SIZE_MISMATCH, out, pos);   // LZ4.Frame.cs:152-155
        if (f.flg & 4) {
            if (pos + 4 > len) return stream_outcome(ALZ_ST_INPUT_TRUNCATED, out, pos);
            v.content_checksum(frame_start, out, pos);
            pos += 4;
        }
    }
    return stream_outcome(ALZ_ST_OK, out, pos);
}

// ---- Snappy
struct SnappyReader { size_t pos; uint64_t out; uint32_t clen; };                        // the in-order reader: where it stands, what it has produced; clen: the declared length of the chunk that is out

// Snappy.Decompress  Formats/Common/Snappy.cs:39-69 over measured chunk sizes.  The managed reader continues wherever a chunk's body stopped, so
// where the next chunk lies depends on the chunk before it; nearly always that is where the chunk's declared length says.  The chunks are
// collected on that assumption (measure(body offset): a body is given the rest of the file, as the reader gives it -- it stops at its declared
// size by itself) ...
template <class Measure>
inline void snappy_measure_collect(const uint8_t* src, size_t len, size_t pos, Measure measure) {
    while (pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, pos);
        if (c.kind == SnappyChunk::TRUNCATED || c.kind == SnappyChunk::RESERVED) break;
        if (c.kind == SnappyChunk::COMPRESSED) measure(c.body);
        pos = c.next;
    }
}
// ... and the reader is replayed over the results `rs` of the `n` bodies `ss` (file_off: where the file lies in their source): it follows
// the measured src_used.  True: the outcome is in `o`.  False: it has left the assumed places -- collect again from r.pos.
inline bool snappy_measure_replay(const uint8_t* src, size_t len, uint64_t cap, SnappyReader& r, uint64_t file_off, const alz_stream* ss, size_t n,
                                  const alz_result* rs, Outcome& o) {
    int32_t st = ALZ_ST_OK; size_t k = 0;
    while (r.pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, r.pos);
        if (c.kind == SnappyChunk::TRUNCATED) { r.pos = c.next; st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { o = refused(ALZ_E_FORMAT); return true; }
        if (c.kind == SnappyChunk::COMPRESSED) {
            if (k >= n || ss[k].src_off != file_off + c.body) {                          // the chunk before ended elsewhere than it declared
                if (k == 0) { o = refused(ALZ_E_INVALID); return true; }                 // (cannot happen: the first chunk is where the collection started)
                return false;
            }
            const alz_result& m = rs[k++];
            const int32_t cs = place_body(m, r.out, cap);
            r.pos = c.body + m.src_used;
            if (cs != ALZ_ST_OK) { st = cs; break; }
        } else if (c.kind == SnappyChunk::STORED) {
            r.pos = c.body;
            if (r.out + c.stored > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
            r.out += c.stored; r.pos = c.next;
        } else r.pos = c.next;
    }
    o = stream_outcome(st, r.out, r.pos);
    return true;
}

// A decoder lays the chunks out at the places they declare: a piece is a compressed or a stored chunk, in file order.  A compressed piece is
// decoded at `at` into `cap` bytes (its declared size `n`, clipped to the destination); a stored piece is `n` bytes from `off` for `out`.
struct SnappyPiece { bool stored; size_t hdr, off; uint32_t n, clen; uint64_t out, at; uint32_t cap; };
struct SnappyLayout {
    std::vector<SnappyPiece> pieces;
    bool reserved = false;                                                               // the walk ended at a reserved chunk: E_FORMAT once reached
    int32_t walk_st = ALZ_ST_OK;
    size_t pos = 10; uint64_t out = 0;                                                   // where the walk ended; the declared sizes
};
// Every layer that copies stored chunks hands in a sink: sink.stored(off, out, n) -- n > 0 bytes of the file from `off` belong at `out` of the
// output, and fit.  The layout reports the stored pieces at their declared places, the in-order reader those it passes.
template <class Sink>
inline void snappy_layout(const uint8_t* src, size_t len, uint64_t cap, SnappyLayout& w, Sink& sink) {
    while (w.pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, w.pos);
        w.pos = c.next;
        if (c.kind == SnappyChunk::TRUNCATED) { w.walk_st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { w.reserved = true; break; }
        if (c.kind == SnappyChunk::COMPRESSED) {
            const uint32_t size = snappy_varint(src + c.body, len - c.body, nullptr);
            const uint64_t out = w.out;
            w.pieces.push_back(SnappyPiece{ false, c.hdr, c.body, size, c.len, out, out < cap ? out : cap, clamp32((size_t)(out < cap ? (cap - out < size ? cap - out : size) : 0)) });
            w.out += size;
        } else if (c.kind == SnappyChunk::STORED) {
            w.pieces.push_back(SnappyPiece{ true, c.hdr, c.body, c.stored, c.len, w.out, w.out, 0 });
            if (w.out + c.stored <= cap && c.stored) sink.stored(c.body, w.out, c.stored);
            w.out += c.stored;
        }
    }
}
// The first failing piece in file order, compressed or stored, decides status and length; result(k): what the k-th compressed piece
// returned.  The managed decoder continues wherever a chunk's body stopped; a chunk whose body does not end at its declared length is
// refused here (ALZ_E_FORMAT).  True: the outcome is in `o`.  False: a chunk decodes to more than it declares (its last element runs past
// the size), which moves every chunk behind it -- on in order with `r`, which stands at that chunk.
template <class Results>
inline bool snappy_judge(const SnappyLayout& w, uint64_t cap, Results result, SnappyReader& r, Outcome& o) {
    uint64_t produced = w.out < cap ? w.out : cap; int32_t fst = ALZ_ST_OK; size_t k = 0;
    for (const SnappyPiece& p : w.pieces) {
        if (p.stored) {
            if (p.out + p.n > cap) { fst = ALZ_ST_OUTPUT_CAPACITY; produced = p.out; break; }
            continue;
        }
        const alz_result& g = result(k++);
        int32_t cs = g.status;
        if (cs == ALZ_ST_OUTPUT_CAPACITY && p.cap == p.n && p.at + (uint64_t)p.n < cap) { r = SnappyReader{ p.hdr, p.at, 0 }; return false; }
        if (cs == ALZ_ST_OK && g.dst_len < p.n) cs = ALZ_ST_OUTPUT_CAPACITY;             // the declared size did not fit dst
        if (cs == ALZ_ST_OK && (uint64_t)g.src_used + 4 != p.clen) { o = refused(ALZ_E_FORMAT); return true; }
        if (cs != ALZ_ST_OK) { fst = cs; produced = p.at + g.dst_len; break; }
    }
    if (fst == ALZ_ST_OK && w.reserved) { o = refused(ALZ_E_FORMAT); return true; }
    if (fst == ALZ_ST_OK && w.walk_st != ALZ_ST_OK) fst = w.walk_st;
    o = stream_outcome(fst, produced, w.pos);
    return true;
}
// The in-order reader, one compressed chunk per call: takes in what the chunk that was out returned (got; NULL at the start), then reads on.
// True: the outcome is in `o`.  False: the body at r.pos is to be decoded at r.out, into all the room there is.
template <class Sink>
inline bool snappy_read_on(const uint8_t* src, size_t len, uint64_t cap, SnappyReader& r, const alz_result* got, Sink& sink, Outcome& o) {
    int32_t st = ALZ_ST_OK;
    if (got) {
        r.out += got->dst_len;
        if (got->status != ALZ_ST_OK) st = got->status;
        else if ((uint64_t)got->src_used + 4 != r.clen) { o = refused(ALZ_E_FORMAT); return true; }   // (as the judge: a body that does not end at the declared length)
        else r.pos += got->src_used;
    }
    while (st == ALZ_ST_OK && r.pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, r.pos);
        r.pos = c.body;
        if (c.kind == SnappyChunk::TRUNCATED) { st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { o = refused(ALZ_E_FORMAT); return true; }
        if (c.kind == SnappyChunk::COMPRESSED) { r.clen = c.len; return false; }
        if (c.kind == SnappyChunk::STORED) {
            if (r.out + c.stored > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
            if (c.stored) sink.stored(c.body, r.out, c.stored);
            r.out += c.stored;
        }
        r.pos = c.next;
    }
    o = stream_outcome(st, r.out, r.pos);
    return true;
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
