// alz_container_measure.cpp -- alz_container_measure: the decompressed size of a file of a container WITHOUT a size field (PRS, LZO, FastLZ, LZ4 frame /
// legacy, framed Snappy) from its bodies measured on the GPU (alz_measure_batch).  The framing of the LZ4 and Snappy files is read by alz_framing.h, the
// same code alz_container.cpp's decoders read it with; this file is a translation unit of its own because it calls into the batch half of the library,
// which the header parsers of alz_container.cpp are built without (their sanitized fuzz binary).
#include <cstdint>
#include <cstring>
#include <vector>

#include "alz_framing.h"
#include "alz_measure.h"
#include "auroralz.h"

namespace {

using namespace alz_framing;

// ---------------------------------------------------------------------------------------------- sizes without decoding (alz_container_measure)
// A body measured with no bound on its count (alz_measure_batch, dst_cap = kNoBound) tells what it does in ANY destination: with `room` bytes left it
// ends as measured when its bytes fit, and in OUTPUT_CAPACITY with the room used up otherwise (the first token that does not fit stops the decoder, in
// front of any later error).  So the bodies of a file go out as ONE batch, and the in-order reader is replayed over the results on the host.
const uint32_t kNoBound = 0xFFFFFF00u;
inline alz_stream measured_body(uint32_t fmt, size_t off, size_t n) {
    alz_stream s; memset(&s, 0, sizeof(s));
    s.src_off = off; s.src_len = clamp32(n); s.dst_cap = kNoBound; s.format = fmt;
    return s;
}
// advances `out` by what the body leaves in a destination of `cap` bytes; returns its status there
inline int32_t place_body(const alz_result& m, uint64_t& out, uint64_t cap) {
    const uint64_t room = out < cap ? cap - out : 0;
    if (m.dst_len > room) { out += room; return ALZ_ST_OUTPUT_CAPACITY; }
    out += m.dst_len;
    return m.status;
}

// LZ4.Decompress  Formats/Common/LZ4.cs:50-93 as the in-order reader sees the file, over measured block sizes.  The frames are read once (alz_framing.h:
// where a block lies does not depend on what any block decodes to), their compressed blocks go out as ONE measure batch, and the reader is replayed over
// the results: blocks in file order, then what the frame's read met behind them.  Blocks of a linked frame are measured like independent ones: history
// only supplies bytes, never sizes.  The content checksum is taken as correct.
int lz4_file_measure(alz_ctx* ctx, const uint8_t* src, size_t len, size_t cap, size_t* size_out, size_t* src_used, int32_t* status) {
    std::vector<Lz4Frame> frames; std::vector<Lz4Block> blocks; std::vector<alz_stream> ss; std::vector<alz_result> rs;
    size_t pos = 0; uint32_t magic = 0;
    while (magic != 0 || pos < len) {
        frames.emplace_back(); Lz4Frame& f = frames.back();
        lz4_read_frame(src, len, pos, magic, f, blocks);
        pos = f.end; magic = f.next_magic;
        for (const Lz4Block* b = blocks.data() + f.first, *e = b + f.count; b != e; b++) if (!b->raw) ss.push_back(measured_body(ALZ_FMT_LZ4_BLOCK, b->off, b->len));
        if (f.fault != ALZ_OK || f.truncated || f.ends_file) break;
        if (f.flg & 4) { if (pos + 4 > len) break; pos += 4; }                               // content checksum: needs the bytes
    }
    rs.resize(ss.size());
    if (!ss.empty()) { const int e = alz_measure_batch(ctx, nullptr, (uint32_t)ss.size(), src, len, ss.data(), rs.data()); if (e != ALZ_OK) return e; }
    uint64_t out = 0; int32_t st = ALZ_ST_OK; int rc = ALZ_OK; size_t k = 0; pos = 0;
    for (const Lz4Frame& f : frames) {
        const uint64_t frame_start = out;
        for (const Lz4Block* b = blocks.data() + f.first, *e = b + f.count; b != e; b++) {
            if (!b->raw) st = place_body(rs[k++], out, cap);
            else {                                                                           // what fits, as the window writes it
                const uint64_t room = out < cap ? cap - out : 0;
                if (b->len > room) { out += room; st = ALZ_ST_OUTPUT_CAPACITY; } else out += b->len;
            }
            if (st != ALZ_ST_OK) { pos = f.behind(*b); break; }
        }
        if (st != ALZ_ST_OK) break;
        pos = f.end;
        if ((rc = f.fault) != ALZ_OK) break;
        if (f.truncated) { st = ALZ_ST_INPUT_TRUNCATED; break; }
        if ((f.flg & 8) && out - frame_start != f.content) { st = ALZ_ST_OUTPUT_SIZE_MISMATCH; break; }   // LZ4.Frame.cs:152-155
        if (f.flg & 4) { if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; } pos += 4; }
    }
    if (size_out) *size_out = (size_t)out;
    if (src_used) *src_used = pos;
    if (status) *status = st;
    if (rc != ALZ_OK) return rc;
    return st == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}

// Snappy.Decompress  Formats/Common/Snappy.cs:39-69 over measured chunk sizes.  The managed reader continues wherever a chunk's body stopped, so where
// the next chunk lies depends on the chunk before it; nearly always that is where the chunk's declared length says.  The chunks are collected on that
// assumption and measured as one batch (a body is given the rest of the file, as the reader gives it: it stops at its declared size by itself); the
// replay follows the measured src_used, and where it leaves the assumed positions the rest of the file is collected again from there.
int snappy_file_measure(alz_ctx* ctx, const uint8_t* src, size_t len, size_t cap, size_t* size_out, size_t* src_used, int32_t* status) {
    if (len < 10 || memcmp(src, kSnappyId, 10)) return ALZ_E_FORMAT;
    size_t pos = 10; uint64_t out = 0; int32_t st = ALZ_ST_OK;
    std::vector<alz_stream> ss; std::vector<alz_result> rs;
    for (bool more = true; more;) {
        more = false;
        ss.clear();
        for (size_t q = pos; q < len;) {
            const SnappyChunk c = snappy_read_chunk(src, len, q);
            if (c.kind == SnappyChunk::TRUNCATED || c.kind == SnappyChunk::RESERVED) break;
            if (c.kind == SnappyChunk::COMPRESSED) ss.push_back(measured_body(ALZ_FMT_SNAPPY_RAW, c.body, len - c.body));
            q = c.next;
        }
        rs.resize(ss.size());
        if (!ss.empty()) { const int e = alz_measure_batch(ctx, nullptr, (uint32_t)ss.size(), src, len, ss.data(), rs.data()); if (e != ALZ_OK) return e; }
        size_t k = 0;
        while (pos < len) {
            const SnappyChunk c = snappy_read_chunk(src, len, pos);
            if (c.kind == SnappyChunk::TRUNCATED) { pos = c.next; st = ALZ_ST_INPUT_TRUNCATED; break; }
            if (c.kind == SnappyChunk::RESERVED) return ALZ_E_FORMAT;
            if (c.kind == SnappyChunk::COMPRESSED) {
                if (k >= ss.size() || ss[k].src_off != c.body) {                             // the chunk before ended elsewhere than it declared
                    if (k == 0) return ALZ_E_INVALID;                                        // (cannot happen: the first chunk is where the collection started)
                    more = true; break;
                }
                const alz_result& m = rs[k++];
                const int32_t cs = place_body(m, out, cap);
                pos = c.body + m.src_used;
                if (cs != ALZ_ST_OK) { st = cs; break; }
            } else if (c.kind == SnappyChunk::STORED) {
                pos = c.body;
                if (out + c.stored > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
                out += c.stored; pos = c.next;
            } else pos = c.next;
        }
    }
    if (size_out) *size_out = (size_t)out;
    if (src_used) *src_used = pos;
    if (status) *status = st;
    return st == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}

}  // namespace

extern "C" {

// Decompressed size of a file of a container without a size field, by measuring its bodies on the GPU (include/auroralz.h)
int alz_container_measure(alz_ctx* ctx, uint32_t container, const alz_container_options* opt, const uint8_t* src, size_t len, size_t size_limit,
                          size_t* size_out, size_t* src_used, int32_t* status) {
    (void)opt;
    if (!ctx || !src) return ALZ_E_INVALID;
    alz_stream ss[2]; alz_result rs[2]; uint32_t n = 1;
    switch (container) {
    case ALZ_C_PRS: {                                                                       // PRS.cs:42-57: the detected byte order, then the other one
        const bool first_big = alz_host_prs_byte_order(src, len) == 2;
        ss[0] = measured_body(first_big ? ALZ_FMT_PRS_BE : ALZ_FMT_PRS_LE, 0, len);
        ss[1] = measured_body(first_big ? ALZ_FMT_PRS_LE : ALZ_FMT_PRS_BE, 0, len);
        n = 2;
        break;
    }
    case ALZ_C_LZO: ss[0] = measured_body(ALZ_FMT_LZO, 0, len); break;                      // LZO.cs:42-43
    case ALZ_C_FASTLZ: ss[0] = measured_body(ALZ_FMT_FASTLZ, 0, len); break;                // FastLZ.cs:40-52
    case ALZ_C_LZ4_LEGACY: case ALZ_C_LZ4_FRAME: return lz4_file_measure(ctx, src, len, size_limit, size_out, src_used, status);
    case ALZ_C_SNAPPY: return snappy_file_measure(ctx, src, len, size_limit, size_out, src_used, status);
    default: return ALZ_E_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; i++) ss[i].dst_cap = clamp32(size_limit);                   // (one body: the limit is its capacity, as run_body passes it)
    const int rc = alz_measure_batch(ctx, nullptr, n, src, len, ss, rs);
    if (rc != ALZ_OK) return rc;
    const alz_result& r = (n == 2 && rs[0].status != ALZ_ST_OK) ? rs[1] : rs[0];
    if (size_out) *size_out = r.dst_len;
    if (src_used) *src_used = r.src_used;
    if (status) *status = r.status;
    return r.status == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}

}  // extern "C"
