// alz_container_measure.cpp -- alz_container_measure: the decompressed size of a file of a container WITHOUT a size field (PRS, LZO, FastLZ, LZ4 frame /
// legacy, framed Snappy) from its bodies measured on the GPU (alz_measure_batch).  The framing walks are those of alz_container.cpp's decoders (cited per
// function, paths relative to the reference's src); this file is a translation unit of its own because it calls into the batch half of the library, which the
// header parsers of alz_container.cpp are built without (their sanitized fuzz binary).
#include <cstdint>
#include <cstring>
#include <vector>

#include "alz_measure.h"
#include "auroralz.h"

namespace {

inline uint32_t le32(const uint8_t* p) { return ((uint32_t)p[3] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0]; }
inline uint32_t clamp32(size_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }
const uint8_t kSnappyId[10] = { 0xff, 0x06, 0x00, 0x00, 0x73, 0x4e, 0x61, 0x50, 0x70, 0x59 };                // Snappy.cs:17
inline bool lz4_magic_defined(uint32_t v) { return v == 0x184C2102u || v == 0x184D2204u || (v >= 0x184D2A50u && v <= 0x184D2A5Fu); }   // LZ4.Frame.cs:50-70

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

// LZ4.Decompress  Formats/Common/LZ4.cs:50-93 as the in-order reader sees the file (the walk of lz4_file_decompress: magic, descriptor, block sizes, stored
// blocks, end marks, the declared content size, block checksums), over measured block sizes.  The walk runs twice: once to collect the compressed
// blocks -- where a block lies does not depend on what any block decodes to --, then, behind ONE measure batch, to replay the reader.  Blocks of a linked
// frame are measured like independent ones: history only supplies bytes, never sizes.  The content checksum is taken as correct.
int lz4_file_measure(alz_ctx* ctx, const uint8_t* src, size_t len, size_t cap, size_t* size_out, size_t* src_used, int32_t* status) {
    std::vector<alz_stream> ss; std::vector<alz_result> rs;
    size_t pos = 0; uint64_t out = 0; int32_t st = ALZ_ST_OK;
    auto walk = [&](bool collect) -> int {
        size_t k = 0; int rc = ALZ_OK; bool done = false;
        pos = 0; out = 0; st = ALZ_ST_OK;
        auto body = [&](size_t off, uint32_t n) {
            if (collect) { ss.push_back(measured_body(ALZ_FMT_LZ4_BLOCK, off, n)); return; }
            const int32_t bst = place_body(rs[k++], out, cap);
            if (bst != ALZ_ST_OK) st = bst;
        };
        while (pos < len && st == ALZ_ST_OK && rc == ALZ_OK && !done) {
            if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
            uint32_t magic = le32(src + pos); pos += 4;
            for (bool again = true; again && st == ALZ_ST_OK && rc == ALZ_OK && !done;) {
                again = false;
                if (magic == 0x184C2102u) {                                                  // legacy  LZ4.cs:96-111
                    if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                    uint32_t bs = le32(src + pos); pos += 4;
                    bool next = false;
                    for (;;) {
                        if (bs > len - pos) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                        body(pos, bs); pos += bs;
                        if (st != ALZ_ST_OK) break;
                        if (pos >= len) break;                                               // ReadByte() == -1
                        if (src[pos] == 0xFF) { pos++; done = true; break; }                 // the EOF flag: Decompress returns
                        if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                        bs = le32(src + pos); pos += 4;
                        if (lz4_magic_defined(bs)) { next = true; break; }
                    }
                    if (st != ALZ_ST_OK || done) break;
                    if (next) { magic = bs; again = true; } else done = true;                // blockSize == 0: Decompress returns
                } else if (magic == 0x184D2204u) {                                           // frame  LZ4.Frame.cs:107-174
                    const uint64_t frame_start = out;
                    if (pos + 2 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                    const uint32_t flg = src[pos], bd = src[pos + 1]; pos += 2;
                    uint32_t bmax;
                    switch ((bd & 0x70) >> 4) { case 4: bmax = 0x10000; break; case 5: bmax = 0x40000; break; case 6: bmax = 0x100000; break; case 7: bmax = 0x400000; break; default: bmax = 0; break; }
                    if (bmax == 0) { rc = ALZ_E_FORMAT; break; }
                    uint64_t content = 0;
                    if (flg & 8) { if (pos + 8 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; } content = (uint64_t)le32(src + pos) | ((uint64_t)le32(src + pos + 4) << 32); pos += 8; }
                    if (flg & 1) { if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; } pos += 4; }
                    if (pos + 1 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                    pos += 1;                                                                // HeaderChecksum: read, not verified
                    if (flg & 1) { rc = ALZ_E_UNSUPPORTED; break; }                          // external dictionaries  LZ4.Frame.cs:113-114
                    for (;;) {
                        if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                        const uint32_t bsz = le32(src + pos); pos += 4;
                        if (bsz == 0) break;                                                 // EndMark
                        const bool raw = (bsz & 0x80000000u) != 0; const uint32_t n = bsz & 0x7FFFFFFFu;
                        if (n > bmax) { rc = ALZ_E_FORMAT; break; }
                        if (n > len - pos) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                        const size_t boff = pos; pos += n;
                        if (flg & 16) {                                                      // block checksum over the stored bytes
                            if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                            if (le32(src + pos) != alz_host_xxh32(src + boff, n, 0)) { rc = ALZ_E_CHECKSUM; break; }
                            pos += 4;
                        }
                        if (!raw) body(boff, n);
                        else if (!collect) {                                                 // what fits, as the window writes it
                            const uint64_t room = out < cap ? cap - out : 0;
                            if (n > room) { out += room; st = ALZ_ST_OUTPUT_CAPACITY; } else out += n;
                        }
                        if (st != ALZ_ST_OK) break;
                    }
                    if (rc != ALZ_OK || st != ALZ_ST_OK) break;
                    if (!collect && (flg & 8) && out - frame_start != content) { st = ALZ_ST_OUTPUT_SIZE_MISMATCH; break; }   // LZ4.Frame.cs:152-155
                    if (flg & 4) { if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; } pos += 4; }                        // content checksum: needs the bytes
                } else if (magic >= 0x184D2A50u && magic <= 0x184D2A5Fu) {                    // skippable
                    if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                    const uint32_t n = le32(src + pos); pos += 4;
                    pos = (uint64_t)pos + n > len ? len : pos + n;
                } else { pos -= 4; done = true; }                                            // not a frame: stop in front of it
            }
        }
        return rc;
    };
    (void)walk(true);
    rs.resize(ss.size());
    if (!ss.empty()) { const int e = alz_measure_batch(ctx, nullptr, (uint32_t)ss.size(), src, len, ss.data(), rs.data()); if (e != ALZ_OK) return e; }
    const int rc = walk(false);
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
        for (size_t q = pos; q + 4 <= len;) {
            const uint32_t type = src[q], cl = (uint32_t)src[q + 1] | ((uint32_t)src[q + 2] << 8) | ((uint32_t)src[q + 3] << 16); q += 4;
            if (type == 0) {
                if (q + 4 > len) break;
                ss.push_back(measured_body(ALZ_FMT_SNAPPY_RAW, q + 4, len - q - 4));
                q = (uint64_t)q + cl > len ? len : q + cl;
            } else if (type == 1) {
                if (q + 4 > len || cl < 4) break;
                q += 4; q += cl - 4 > len - q ? len - q : cl - 4;
            } else {
                if (type >= 0x02 && type <= 0x7F) break;
                q = (uint64_t)q + cl > len ? len : q + cl;
            }
        }
        rs.resize(ss.size());
        if (!ss.empty()) { const int e = alz_measure_batch(ctx, nullptr, (uint32_t)ss.size(), src, len, ss.data(), rs.data()); if (e != ALZ_OK) return e; }
        size_t k = 0;
        while (pos < len) {
            if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
            const uint32_t type = src[pos], cl = (uint32_t)src[pos + 1] | ((uint32_t)src[pos + 2] << 8) | ((uint32_t)src[pos + 3] << 16);
            if (type == 0) {
                if (pos + 8 > len) { pos += 4; st = ALZ_ST_INPUT_TRUNCATED; break; }
                if (k >= ss.size() || ss[k].src_off != pos + 8) {                            // the chunk before ended elsewhere than it declared
                    if (k == 0) return ALZ_E_INVALID;                                        // (cannot happen: the first chunk is where the collection started)
                    more = true; break;
                }
                pos += 8;
                const alz_result& m = rs[k++];
                const int32_t cs = place_body(m, out, cap);
                pos += m.src_used;
                if (cs != ALZ_ST_OK) { st = cs; break; }
            } else if (type == 1) {
                pos += 4;
                if (pos + 4 > len || cl < 4) { st = ALZ_ST_INPUT_TRUNCATED; break; }
                pos += 4;
                uint32_t n = cl - 4; if (n > len - pos) n = (uint32_t)(len - pos);            // SubStream.CopyTo copies what is there
                if (out + n > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
                out += n; pos += n;
            } else {
                pos += 4;
                if (type >= 0x02 && type <= 0x7F) return ALZ_E_FORMAT;                        // reserved unskippable chunk  Snappy.cs:61-62
                pos = (uint64_t)pos + cl > len ? len : pos + cl;
            }
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
