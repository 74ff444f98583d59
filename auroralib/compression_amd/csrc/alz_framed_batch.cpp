// alz_framed_batch.cpp -- LZ4 (frame, legacy) and framed Snappy files in batches: alz_framed_decode_batch / alz_framed_measure_batch.  What
// alz_container_decompress / alz_container_measure do for one such file, for a whole set in one call.  The contract is differential: per
// file the outcome of the single-file call (alz_container.cpp, alz_container_measure.cpp), whose verdict order is restated here over the
// same framing readers (alz_framing.h).  Pure host code on the public ABI plus the XXH32 and range-copy kernels (alz_xxh32.h).
//
// The source is uploaded once and one device destination covers all slots.
//   LZ4     Where a block's output lies depends on what the blocks in front of it decode to, so the compressed blocks of ALL files are
//           measured first (one alz_measure_batch_device: a body measured without a bound tells what it does in any destination).  The
//           in-order reader is replayed over the sizes on the host; that settles every block's place and how far each file is read.  The
//           blocks then decode at their exact places: all blocks that reach into nothing in front of them side by side -- whatever
//           frame or file they belong to --, a block of a linked frame that does reach back one round behind the blocks in front of it.
//   Snappy  Every compressed chunk declares its size, so the chunks of all files go out in the first round at their declared places; a
//           file with a chunk that decodes to more than it declares is read on in order, one chunk per round (snappy_in_order).
// A round is ONE device-resident decode for the steps of all files (split in two plans where a few long blocks would otherwise decode on
// a wavefront each, as the single-file layer splits them).  Stored LZ4 blocks and stored Snappy chunks are copied HBM to HBM by ONE launch
// per round.  The outputs of the frames that carry a content checksum are hashed where they lie by ONE alz_xxh32_batch_device; block
// checksums are verified by the reader over the source bytes in host memory.  The outputs are downloaded once.
// A measure is the same walk without the decode: LZ4 files take one measure batch, a Snappy file one more for every chunk that ends
// elsewhere than it declares (alz_container_measure.cpp).
#include <atomic>
#include <cstring>
#include <vector>

#include "auroralz.h"
#include "alz_file_batch.h"
#include "alz_framing.h"
#include "alz_xxh32.h"

namespace {

using namespace alz_framing;
using namespace alz_file_batch;

const uint32_t kNoBound = 0xFFFFFF00u;                                         // the largest dst_cap of a stream

std::atomic<uint64_t> g_refused{0};                                            // files whose decode did not confirm the measured sizes (alz_debug_framed_batch_refused)

inline bool lz4_container(uint32_t c) { return c == ALZ_C_LZ4_FRAME || c == ALZ_C_LZ4_LEGACY; }
inline uint32_t clamp_cap(uint64_t v) { return v > kNoBound ? kNoBound : (uint32_t)v; }
inline alz_stream body(uint32_t fmt, uint64_t src_off, size_t src_len, uint64_t dst_off, uint32_t dst_cap, uint32_t hist) {
    alz_stream s; memset(&s, 0, sizeof(s));
    s.src_off = src_off; s.src_len = clamp32(src_len); s.dst_off = dst_off; s.dst_cap = dst_cap; s.aux0 = hist; s.format = fmt;
    return s;
}
// advances `out` by what a measured body leaves in a destination of `cap` bytes; returns its status there (alz_container_measure.cpp)
inline int32_t place_body(const alz_result& m, uint64_t& out, uint64_t cap) {
    const uint64_t room = out < cap ? cap - out : 0;
    if (m.dst_len > room) { out += room; return ALZ_ST_OUTPUT_CAPACITY; }
    out += m.dst_len;
    return m.status;
}
// (worth the whole GPU by itself: plan_create's own test, as alz_container.cpp restates it)
inline bool long_block(const alz_stream& s) { return s.format == ALZ_FMT_LZ4_BLOCK && s.src_len >= 8192u && s.dst_cap >= (24u << 10); }

void finish(alz_file_result& r, int rc, int32_t status, uint64_t out, size_t used) {
    const bool delivered = rc == ALZ_OK || rc == ALZ_E_STREAM;                  // (the single-file call leaves its out-parameters unset otherwise)
    r.rc = rc; r.status = delivered ? status : ALZ_ST_OK; r.dst_len = delivered ? (uint32_t)out : 0u; r.src_used = delivered ? (uint32_t)used : 0u;
}

// a compressed block or chunk that goes to the device, and what is known about it beforehand
struct Step {
    uint32_t file, round;
    alz_stream s;
    bool sized;                                                                 // LZ4: the measured size fits and ends OK; the decode has to confirm it
    alz_result got;
};
struct Checked { uint32_t file; uint64_t off; uint32_t len, want; };            // a frame's output and its content checksum word

// ---------------------------------------------------------------------------------------------- LZ4
struct Lz4File { std::vector<Lz4Frame> frames; std::vector<Lz4Block> blocks; size_t first = 0; };   // first: its first compressed block in the measure batch

// LZ4.Decompress  Formats/Common/LZ4.cs:50-93: the frames of the file (where a block lies does not depend on what any block decodes to)
void lz4_walk(const uint8_t* src, size_t len, Lz4File& w, uint64_t file_off, std::vector<alz_stream>& ss) {
    size_t pos = 0; uint32_t magic = 0;
    w.first = ss.size();
    while (magic != 0 || pos < len) {
        w.frames.emplace_back(); Lz4Frame& f = w.frames.back();
        lz4_read_frame(src, len, pos, magic, f, w.blocks);
        pos = f.end; magic = f.next_magic;
        for (const Lz4Block* b = w.blocks.data() + f.first, *e = b + f.count; b != e; b++)
            if (!b->raw) ss.push_back(body(ALZ_FMT_LZ4_BLOCK, file_off + b->off, b->len, 0, kNoBound, 0));
        if (f.fault != ALZ_OK || f.truncated || f.ends_file) break;
        if (f.flg & 4) { if (pos + 4 > len) break; pos += 4; }                  // content checksum: needs the bytes
    }
}

// The in-order reader over the measured sizes `m` (one per compressed block, file order).  measure: the outcome of alz_container_measure in
// `r`.  decode: the outcome of alz_container_decompress as far as the sizes tell it -- the decode of the last step confirms or replaces
// status and length -- with the file's steps, copies and checksummed frames appended; returns the index of the step that ends the file, or -1.
long lz4_replay(uint32_t file, const alz_stream& fs, const uint8_t* src, const Lz4File& w, const alz_result* m, bool decode, alz_file_result& r,
                std::vector<Step>& steps, std::vector<alz_copy_range>& copies, std::vector<Checked>& checked) {
    const size_t len = fs.src_len; const uint64_t cap = fs.dst_cap;
    uint64_t out = 0; int32_t st = ALZ_ST_OK; int rc = ALZ_OK; size_t pos = 0, k = 0; long last = -1;
    for (const Lz4Frame& f : w.frames) {
        const uint64_t frame_start = out;
        // one LzWindows serves all blocks of a frame whatever its flag says (alz_container.cpp): a frame is linked when a block reaches back
        bool linked = false;
        if (decode && f.kind == Lz4Frame::FRAME)
            for (size_t i = 1; !linked && i < f.count; i++) { const Lz4Block& b = w.blocks[f.first + i]; linked = !b.raw && lz4_block_reaches_back(src + b.off, b.len); }
        uint32_t rounds = 0;                                                    // rounds the compressed blocks of this frame in front of a block take
        for (const Lz4Block* b = w.blocks.data() + f.first, *e = b + f.count; b != e; b++) {
            const uint64_t room = cap - out;
            if (b->raw) {                                                       // what fits, as the window writes it
                const uint64_t n = b->len > room ? room : b->len;
                if (decode && n) copies.push_back(alz_copy_range{fs.src_off + b->off, fs.dst_off + out, (uint32_t)n, 0});
                out += n;
                if (n < b->len) st = ALZ_ST_OUTPUT_CAPACITY;
            } else {
                const alz_result& mb = m[k++];
                if (decode) {
                    const uint64_t hist = linked ? out - frame_start : 0;
                    if (linked && (uint64_t)clamp32((size_t)room) + hist > 0xFFFFFF00ull) { finish(r, ALZ_E_UNSUPPORTED, 0, 0, 0); return -1; }
                    Step s; s.file = file; s.sized = mb.status == ALZ_ST_OK && mb.dst_len <= room;
                    // a block behind others of a linked frame waits for them only if it reads them
                    const bool waits = linked && b != w.blocks.data() + f.first && lz4_block_reaches_back(src + b->off, b->len);
                    s.round = waits ? rounds : 0;
                    rounds = s.round + 1 > rounds ? s.round + 1 : rounds;
                    s.s = body(ALZ_FMT_LZ4_BLOCK, fs.src_off + b->off, b->len, fs.dst_off + out, s.sized ? mb.dst_len : clamp_cap(room), (uint32_t)hist);
                    memset(&s.got, 0, sizeof(s.got));
                    steps.push_back(s);
                }
                st = place_body(mb, out, cap);
                if (decode && st != ALZ_ST_OK) last = (long)steps.size() - 1;
            }
            if (st != ALZ_ST_OK) { pos = decode ? f.end : f.behind(*b); break; }
        }
        if (st != ALZ_ST_OK) break;
        pos = f.end;
        if ((rc = f.fault) != ALZ_OK) break;
        if (f.truncated) { st = ALZ_ST_INPUT_TRUNCATED; break; }
        if ((f.flg & 8) && out - frame_start != f.content) { st = ALZ_ST_OUTPUT_SIZE_MISMATCH; break; }   // LZ4.Frame.cs:152-155
        if (f.flg & 4) {
            if (pos + 4 > len) { st = ALZ_ST_INPUT_TRUNCATED; break; }
            if (decode) checked.push_back(Checked{file, fs.dst_off + frame_start, (uint32_t)(out - frame_start), le32(src + pos)});
            pos += 4;
        }
    }
    if (rc != ALZ_OK) finish(r, rc, 0, 0, 0);
    else finish(r, st == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM, st, out, pos);
    return last;
}

// ---------------------------------------------------------------------------------------------- Snappy
struct SnappyPiece { bool stored; size_t hdr, off; uint32_t n, clen; uint64_t out; long step; };   // a chunk of the first round, file order
struct SnappyFile {
    bool active = false, in_order = false, reserved = false;
    int32_t walk_st = ALZ_ST_OK;
    size_t pos = 0; uint64_t out = 0;                                           // the walk's end and the declared sizes; in order / measure: the reader's position and output
    std::vector<SnappyPiece> pieces;
    uint32_t wait_clen = 0; long wait_step = -1;                                // in order: the chunk that is out on the device
    size_t first = 0, count = 0;                                                // measure: this round's bodies in the batch
};

// Snappy.Decompress  Formats/Common/Snappy.cs:39-69 as snappy_file_decompress collects it: all chunks at their declared places
void snappy_open(uint32_t file, const alz_stream& fs, const uint8_t* src, SnappyFile& w, alz_file_result& r, std::vector<Step>& steps, std::vector<alz_copy_range>& copies) {
    const size_t len = fs.src_len; const uint64_t cap = fs.dst_cap;
    if (len < 10 || memcmp(src, kSnappyId, 10)) { finish(r, ALZ_E_FORMAT, 0, 0, 0); return; }
    size_t pos = 10; uint64_t out = 0;
    while (pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, pos);
        pos = c.next;
        if (c.kind == SnappyChunk::TRUNCATED) { w.walk_st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { w.reserved = true; break; }      // E_FORMAT once reached
        if (c.kind == SnappyChunk::COMPRESSED) {
            const uint32_t size = snappy_varint(src + c.body, len - c.body, nullptr);
            Step s; s.file = file; s.round = 0; s.sized = false; memset(&s.got, 0, sizeof(s.got));
            s.s = body(ALZ_FMT_SNAPPY_RAW, fs.src_off + c.body, len - c.body, fs.dst_off + (out < cap ? out : cap),
                       clamp32((size_t)(out < cap ? (cap - out < size ? cap - out : size) : 0)), 0);
            w.pieces.push_back(SnappyPiece{false, c.hdr, c.body, size, c.len, out, (long)steps.size()});
            steps.push_back(s);
            out += size;
        } else if (c.kind == SnappyChunk::STORED) {
            w.pieces.push_back(SnappyPiece{true, c.hdr, c.body, c.stored, c.len, out, -1});
            if (out + c.stored <= cap && c.stored) copies.push_back(alz_copy_range{fs.src_off + c.body, fs.dst_off + out, c.stored, 0});
            out += c.stored;
        }
    }
    w.pos = pos; w.out = out; w.active = true;
}

// the first failing chunk in file order, compressed or stored, decides status and length (snappy_file_decompress)
void snappy_judge(const alz_stream& fs, SnappyFile& w, alz_file_result& r, const std::vector<Step>& steps) {
    const uint64_t cap = fs.dst_cap;
    uint64_t produced = w.out < cap ? w.out : cap; int32_t fst = ALZ_ST_OK;
    for (const SnappyPiece& p : w.pieces) {
        if (p.stored) {
            if (p.out + p.n > cap) { fst = ALZ_ST_OUTPUT_CAPACITY; produced = p.out; break; }
            continue;
        }
        const Step& s = steps[(size_t)p.step];
        const uint64_t at = s.s.dst_off - fs.dst_off;
        int32_t cs = s.got.status;
        if (cs == ALZ_ST_OUTPUT_CAPACITY && s.s.dst_cap == p.n && at + (uint64_t)p.n < cap) {   // it decodes to more than it declares: on in order from this chunk
            w.in_order = true; w.pos = p.hdr; w.out = at;
            return;
        }
        if (cs == ALZ_ST_OK && s.got.dst_len < p.n) cs = ALZ_ST_OUTPUT_CAPACITY;                 // the declared size did not fit dst
        if (cs == ALZ_ST_OK && (uint64_t)s.got.src_used + 4 != p.clen) { w.active = false; finish(r, ALZ_E_FORMAT, 0, 0, 0); return; }
        if (cs != ALZ_ST_OK) { fst = cs; produced = at + s.got.dst_len; break; }
    }
    w.active = false;
    if (fst == ALZ_ST_OK && w.reserved) { finish(r, ALZ_E_FORMAT, 0, 0, 0); return; }
    if (fst == ALZ_ST_OK && w.walk_st != ALZ_ST_OK) fst = w.walk_st;
    finish(r, fst == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM, fst, produced, w.pos);
}

// snappy_in_order, one compressed chunk per call: takes in what the chunk on the device returned, then reads on to the next one
void snappy_step(uint32_t file, uint32_t round, const alz_stream& fs, const uint8_t* src, SnappyFile& w, alz_file_result& r, std::vector<Step>& steps,
                 std::vector<alz_copy_range>& copies) {
    const size_t len = fs.src_len; const uint64_t cap = fs.dst_cap;
    int32_t st = ALZ_ST_OK;
    if (w.wait_step >= 0) {
        const alz_result& g = steps[(size_t)w.wait_step].got;
        w.wait_step = -1;
        w.out += g.dst_len;
        if (g.status != ALZ_ST_OK) st = g.status;
        else if ((uint64_t)g.src_used + 4 != w.wait_clen) { w.active = false; finish(r, ALZ_E_FORMAT, 0, 0, 0); return; }
        else w.pos += g.src_used;
    }
    while (st == ALZ_ST_OK && w.pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, w.pos);
        w.pos = c.body;
        if (c.kind == SnappyChunk::TRUNCATED) { st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { w.active = false; finish(r, ALZ_E_FORMAT, 0, 0, 0); return; }
        if (c.kind == SnappyChunk::COMPRESSED) {
            Step s; s.file = file; s.round = round; s.sized = false; memset(&s.got, 0, sizeof(s.got));
            s.s = body(ALZ_FMT_SNAPPY_RAW, fs.src_off + w.pos, len - w.pos, fs.dst_off + w.out, clamp_cap(w.out < cap ? cap - w.out : 0), 0);
            w.wait_step = (long)steps.size(); w.wait_clen = c.len;
            steps.push_back(s);
            return;
        }
        if (c.kind == SnappyChunk::STORED) {
            if (w.out + c.stored > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
            if (c.stored) copies.push_back(alz_copy_range{fs.src_off + w.pos, fs.dst_off + w.out, c.stored, 0});
            w.out += c.stored;
        }
        w.pos = c.next;
    }
    w.active = false;
    finish(r, st == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM, st, w.out, w.pos);
}

// snappy_file_measure, one round: the bodies from the reader's position on, at the places their chunks declare
void snappy_measure_collect(const alz_stream& fs, const uint8_t* src, SnappyFile& w, std::vector<alz_stream>& ss) {
    const size_t len = fs.src_len;
    w.first = ss.size();
    for (size_t q = w.pos; q < len;) {
        const SnappyChunk c = snappy_read_chunk(src, len, q);
        if (c.kind == SnappyChunk::TRUNCATED || c.kind == SnappyChunk::RESERVED) break;
        if (c.kind == SnappyChunk::COMPRESSED) ss.push_back(body(ALZ_FMT_SNAPPY_RAW, fs.src_off + c.body, len - c.body, 0, kNoBound, 0));
        q = c.next;
    }
    w.count = ss.size() - w.first;
}
// ... and the reader replayed over their results: it follows the measured src_used, and stays active where it leaves the assumed places
int snappy_measure_replay(const alz_stream& fs, const uint8_t* src, SnappyFile& w, alz_file_result& r, const alz_stream* ss, const alz_result* rs) {
    const size_t len = fs.src_len; const uint64_t cap = fs.dst_cap;
    int32_t st = ALZ_ST_OK; size_t k = 0;
    while (w.pos < len) {
        const SnappyChunk c = snappy_read_chunk(src, len, w.pos);
        if (c.kind == SnappyChunk::TRUNCATED) { w.pos = c.next; st = ALZ_ST_INPUT_TRUNCATED; break; }
        if (c.kind == SnappyChunk::RESERVED) { w.active = false; finish(r, ALZ_E_FORMAT, 0, 0, 0); return ALZ_OK; }
        if (c.kind == SnappyChunk::COMPRESSED) {
            if (k >= w.count || ss[k].src_off != fs.src_off + c.body) {         // the chunk before ended elsewhere than it declared
                if (k == 0) return ALZ_E_INVALID;                               // (cannot happen: the first chunk is where the collection started)
                return ALZ_OK;                                                  // another round, from here
            }
            const alz_result& m = rs[k++];
            const int32_t cs = place_body(m, w.out, cap);
            w.pos = c.body + m.src_used;
            if (cs != ALZ_ST_OK) { st = cs; break; }
        } else if (c.kind == SnappyChunk::STORED) {
            w.pos = c.body;
            if (w.out + c.stored > cap) { st = ALZ_ST_OUTPUT_CAPACITY; break; }
            w.out += c.stored; w.pos = c.next;
        } else w.pos = c.next;
    }
    w.active = false;
    finish(r, st == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM, st, w.out, w.pos);
    return ALZ_OK;
}

// ---------------------------------------------------------------------------------------------- the device side of a round
int run_plan(alz_ctx* ctx, std::vector<alz_stream>& ss, std::vector<alz_result>& rs, const void* d_src, void* d_dst) {
    alz_plan* pl = nullptr; rs.resize(ss.size());
    int e = alz_plan_create(ctx, nullptr, (uint32_t)ss.size(), ss.data(), &pl);
    if (e != ALZ_OK) return e;
    e = alz_plan_execute(ctx, pl, d_src, d_dst, nullptr);
    if (e == ALZ_OK) e = alz_plan_results(ctx, pl, rs.data());
    alz_plan_destroy(ctx, pl);
    return e;
}
// the steps of round `round`: one plan -- two when a few long blocks stand among short ones (a plan takes its streams one after the other on
// the whole GPU only when all of them are worth it)
int run_round(alz_ctx* ctx, std::vector<Step>& steps, size_t from, uint32_t round, const void* d_src, void* d_dst) {
    std::vector<size_t> ia, ib; std::vector<alz_stream> sa, sb; std::vector<alz_result> ra, rb;
    for (size_t k = from; k < steps.size(); k++) {
        if (steps[k].round != round) continue;
        if (long_block(steps[k].s)) { sa.push_back(steps[k].s); ia.push_back(k); } else { sb.push_back(steps[k].s); ib.push_back(k); }
    }
    if (sa.empty() || sb.empty() || sa.size() > 32) { sb.insert(sb.end(), sa.begin(), sa.end()); ib.insert(ib.end(), ia.begin(), ia.end()); sa.clear(); ia.clear(); }
    if (!sa.empty()) { if (int e = run_plan(ctx, sa, ra, d_src, d_dst)) return e; }
    if (!sb.empty()) { if (int e = run_plan(ctx, sb, rb, d_src, d_dst)) return e; }
    for (size_t k = 0; k < ia.size(); k++) steps[ia[k]].got = ra[k];
    for (size_t k = 0; k < ib.size(); k++) steps[ib[k]].got = rb[k];
    return ALZ_OK;
}

int check_args(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, uint8_t* dst_base, size_t dst_bytes,
               alz_file_result* results, bool measure) {
    if (!ctx || (n && (!files || !results)) || (src_bytes && !src_base) || (!measure && dst_bytes && !dst_base)) return ALZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (!lz4_container(files[i].format) && files[i].format != ALZ_C_SNAPPY) return ALZ_E_INVALID;
        if (!range_ok(files[i].src_off, files[i].src_len, src_bytes)) return ALZ_E_INVALID;
        if (!measure && !range_ok(files[i].dst_off, files[i].dst_cap, dst_bytes)) return ALZ_E_INVALID;
    }
    return ALZ_OK;
}

int measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, alz_file_result* results) {
    DeviceBuffer d_src(ctx);
    int rc;
    if ((rc = d_src.alloc(src_bytes)) || (src_bytes && (rc = alz_memcpy_h2d(ctx, d_src.p, src_base, src_bytes)))) return rc;
    std::vector<Lz4File> lz4(n); std::vector<SnappyFile> snappy(n);
    std::vector<alz_stream> ss; std::vector<alz_result> rs;
    std::vector<Step> no_steps; std::vector<alz_copy_range> no_copies; std::vector<Checked> no_checked;
    uint32_t active = 0;
    for (uint32_t i = 0; i < n; i++) {
        results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
        const uint8_t* src = src_base + files[i].src_off;
        if (lz4_container(files[i].format)) lz4_walk(src, files[i].src_len, lz4[i], files[i].src_off, ss);
        else if (files[i].src_len < 10 || memcmp(src, kSnappyId, 10)) finish(results[i], ALZ_E_FORMAT, 0, 0, 0);
        else { snappy[i].active = true; snappy[i].pos = 10; snappy_measure_collect(files[i], src, snappy[i], ss); active++; }
    }
    for (bool first = true; first || active; first = false) {
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if (!ss.empty() && (rc = alz_measure_batch_device(ctx, nullptr, (uint32_t)ss.size(), (const uint8_t*)d_src.p, src_bytes, ss.data(), rs.data()))) return rc;
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t* src = src_base + files[i].src_off;
            if (first && lz4_container(files[i].format)) lz4_replay(i, files[i], src, lz4[i], rs.data() + lz4[i].first, false, results[i], no_steps, no_copies, no_checked);
            else if (snappy[i].active) {
                if ((rc = snappy_measure_replay(files[i], src, snappy[i], results[i], ss.data() + snappy[i].first, rs.data() + snappy[i].first))) return rc;
                if (!snappy[i].active) active--;
            }
        }
        ss.clear();
        for (uint32_t i = 0; i < n; i++) if (snappy[i].active) snappy_measure_collect(files[i], src_base + files[i].src_off, snappy[i], ss);
    }
    return ALZ_OK;
}

int decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, uint8_t* dst_base, size_t dst_bytes,
                 alz_file_result* results) {
    DeviceBuffer d_src(ctx), d_dst(ctx);
    int rc;
    if ((rc = d_src.alloc(src_bytes)) || (src_bytes && (rc = alz_memcpy_h2d(ctx, d_src.p, src_base, src_bytes)))) return rc;
    if ((rc = d_dst.alloc(dst_bytes))) return rc;
    const uint8_t* ds = (const uint8_t*)d_src.p; uint8_t* dd = (uint8_t*)d_dst.p;

    // the LZ4 files: sizes first, then every block's place
    std::vector<Lz4File> lz4(n); std::vector<SnappyFile> snappy(n);
    std::vector<Step> steps; std::vector<alz_copy_range> copies; std::vector<Checked> checked;
    std::vector<long> last(n, -1);                                              // LZ4: the step that ends the file short of its last block
    {
        std::vector<alz_stream> ss; std::vector<alz_result> rs;
        for (uint32_t i = 0; i < n; i++) if (lz4_container(files[i].format)) lz4_walk(src_base + files[i].src_off, files[i].src_len, lz4[i], files[i].src_off, ss);
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if (!ss.empty() && (rc = alz_measure_batch_device(ctx, nullptr, (uint32_t)ss.size(), ds, src_bytes, ss.data(), rs.data()))) return rc;
        for (uint32_t i = 0; i < n; i++) {
            results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
            const uint8_t* src = src_base + files[i].src_off;
            if (lz4_container(files[i].format)) last[i] = lz4_replay(i, files[i], src, lz4[i], rs.data() + lz4[i].first, true, results[i], steps, copies, checked);
            else snappy_open(i, files[i], src, snappy[i], results[i], steps, copies);
        }
    }
    uint32_t rounds = 0, active = 0;
    for (const Step& s : steps) if (s.round + 1 > rounds) rounds = s.round + 1;
    for (uint32_t i = 0; i < n; i++) active += snappy[i].active;

    size_t from = 0;                                                            // the steps in front of it are done
    for (uint32_t round = 0; round < rounds || active; round++) {
        if (!copies.empty() && (rc = alz_host_range_copy(ctx, (uint32_t)copies.size(), copies.data(), ds, src_bytes, dd, dst_bytes))) return rc;
        copies.clear();
        const size_t end = steps.size();
        if ((rc = run_round(ctx, steps, from, round, ds, dd))) return rc;
        while (from < end && steps[from].round <= round) from++;
        for (uint32_t i = 0; i < n; i++) {
            SnappyFile& w = snappy[i];
            if (!w.active) continue;
            if (!w.in_order) snappy_judge(files[i], w, results[i], steps);
            if (w.active) snappy_step(i, round + 1, files[i], src_base + files[i].src_off, w, results[i], steps, copies);
            if (!w.active) active--;
        }
    }
    if (!copies.empty() && (rc = alz_host_range_copy(ctx, (uint32_t)copies.size(), copies.data(), ds, src_bytes, dd, dst_bytes))) return rc;

    // LZ4: the decode confirms the sizes; the step that ends a file short tells its status and length
    std::vector<uint8_t> redo(n, 0);
    for (size_t k = 0; k < steps.size(); k++) {
        const Step& s = steps[k];
        if (s.s.format != ALZ_FMT_LZ4_BLOCK) continue;
        if (s.sized ? (s.got.status != ALZ_ST_OK || s.got.dst_len != s.s.dst_cap) : s.got.status == ALZ_ST_OK) redo[s.file] = 1;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (redo[i] || last[i] < 0 || results[i].rc != ALZ_E_STREAM) continue;
        const Step& s = steps[(size_t)last[i]];
        results[i].status = s.got.status;
        results[i].dst_len = (uint32_t)(s.s.dst_off - files[i].dst_off + s.got.dst_len);
    }
    // the content checksums, over the outputs where they lie: the first wrong one in file order decides, in front of anything behind it
    if (!checked.empty()) {
        std::vector<alz_stream> ranges(checked.size()); std::vector<uint32_t> sums(checked.size());
        for (size_t k = 0; k < checked.size(); k++) ranges[k] = body(0, checked[k].off, checked[k].len, 0, 0, 0);
        if ((rc = alz_xxh32_batch_device(ctx, 0, (uint32_t)ranges.size(), dd, dst_bytes, ranges.data(), sums.data()))) return rc;
        for (size_t k = 0; k < checked.size(); k++)
            if (sums[k] != checked[k].want && !redo[checked[k].file] && results[checked[k].file].rc != ALZ_E_CHECKSUM) finish(results[checked[k].file], ALZ_E_CHECKSUM, 0, 0, 0);
    }
    // A decode that does not confirm what the measure kernels counted has no place in the layout above: such a file is read by the
    // single-file layer, on the GPU as well, and counted (none is known; the tests hold the count at 0 over the fuzzed corpus).
    std::vector<std::vector<uint8_t>> again(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!redo[i]) continue;
        g_refused.fetch_add(1, std::memory_order_relaxed);
        again[i].resize((size_t)files[i].dst_cap + 1);
        size_t dl = 0, su = 0; int32_t st = ALZ_ST_OK;
        const int frc = alz_container_decompress(ctx, files[i].format, nullptr, src_base + files[i].src_off, files[i].src_len, again[i].data(), files[i].dst_cap, &dl, &su, &st);
        if (frc == ALZ_E_HIP || frc == ALZ_E_NOMEM || frc == ALZ_E_NO_DEVICE || frc == ALZ_E_INVALID) return frc;
        finish(results[i], frc, st, dl, su);
    }
    std::vector<uint32_t> held(n, 0);                                           // (their bytes are on the host already: kept out of the download)
    for (uint32_t i = 0; i < n; i++) if (redo[i]) { held[i] = results[i].dst_len; results[i].dst_len = 0; }
    rc = download(ctx, n, files, results, dd, dst_base);
    for (uint32_t i = 0; i < n; i++) if (redo[i]) { results[i].dst_len = held[i]; if (held[i]) memcpy(dst_base + files[i].dst_off, again[i].data(), held[i]); }
    return rc;
}

}   // namespace

extern "C" {

int alz_framed_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                            uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (int rc = check_args(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, false)) return rc;
    return n ? decode_batch(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results) : ALZ_OK;
}
int alz_framed_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                             alz_file_result* results) {
    if (int rc = check_args(ctx, n, src_base, src_bytes, files, nullptr, 0, results, true)) return rc;
    return n ? measure_batch(ctx, n, src_base, src_bytes, files, results) : ALZ_OK;
}
// files that alz_framed_decode_batch handed to the single-file layer because their decode did not confirm the measured sizes, process-wide
uint64_t alz_debug_framed_batch_refused(void) { return g_refused.load(std::memory_order_relaxed); }
// the host XXH32 the framing reader and the single-file layer use (alz_framing.h): what tools/bench_framed.py times next to the kernel
uint32_t alz_debug_host_xxh32(const uint8_t* p, size_t len, uint32_t seed) { return xxh32(p, len, seed); }

}   // extern "C"
