// alz_framed_batch.cpp -- LZ4 (frame, legacy) and framed Snappy files in batches: alz_framed_decode_batch / alz_framed_measure_batch.  What
// alz_container_decompress / alz_container_measure do for one such file, for a whole set in one call.  The contract is differential: per
// file the outcome of the single-file call (alz_container.cpp, alz_container_measure.cpp).  What the framing readers' records and the
// bodies' results make of a file is decided by the functions of alz_framing.h that the single-file calls run too (lz4_replay,
// snappy_measure_replay, snappy_layout / snappy_judge / snappy_read_on); this file schedules the bodies and moves the bytes.  Pure host
// code on the public ABI plus the XXH32 and range-copy kernels (alz_xxh32.h).
//
// The source is uploaded once and one device destination covers all slots.
//   LZ4     Where a block's output lies depends on what the blocks in front of it decode to, so the compressed blocks of ALL files are
//           measured first (one alz_measure_batch_device: a body measured without a bound tells what it does in any destination).  The
//           in-order reader is replayed over the sizes on the host; that settles every block's place and how far each file is read.  The
//           blocks then decode at their exact places: all blocks that reach into nothing in front of them side by side -- whatever
//           frame or file they belong to --, a block of a linked frame that does reach back one round behind the blocks in front of it.
//   Snappy  Every compressed chunk declares its size, so the chunks of all files go out in the first round at their declared places; a
//           file with a chunk that decodes to more than it declares is read on in order, one chunk per round (snappy_read_on).
// A round is ONE device-resident decode for the steps of all files (split in two plans where a few long blocks would otherwise decode on
// a wavefront each, as the single-file layer splits them: alz_file_batch.h).  Stored LZ4 blocks and stored Snappy chunks are copied HBM to
// HBM by ONE launch per round.  The outputs of the frames that carry a content checksum are hashed where they lie by ONE
// alz_xxh32_batch_device; block checksums are verified by the reader over the source bytes in host memory.  The outputs are downloaded once.
// A measure is the same walk without the decode: LZ4 files take one measure batch, a Snappy file one more for every chunk that ends
// elsewhere than it declares.
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

std::atomic<uint64_t> g_refused{0};                                            // files whose decode did not confirm the measured sizes (alz_debug_framed_batch_refused)

inline bool lz4_container(uint32_t c) { return c == ALZ_C_LZ4_FRAME || c == ALZ_C_LZ4_LEGACY; }
inline bool framed_container(uint32_t c) { return lz4_container(c) || c == ALZ_C_SNAPPY; }
inline uint32_t clamp_cap(uint64_t v) { return v > kNoBound ? kNoBound : (uint32_t)v; }

void deliver(alz_file_result& r, const Outcome& o) {
    const bool delivered = o.rc == ALZ_OK || o.rc == ALZ_E_STREAM;              // (the single-file call leaves its out-parameters unset otherwise)
    r.rc = o.rc; r.status = delivered ? o.status : ALZ_ST_OK; r.dst_len = delivered ? (uint32_t)o.out : 0u; r.src_used = delivered ? (uint32_t)o.pos : 0u;
}

// a compressed block or chunk that goes to the device, and what is known about it beforehand
struct Step {
    uint32_t file, round;
    alz_stream s;
    bool sized;                                                                 // LZ4: the measured size fits and ends OK; the decode has to confirm it
    alz_result got;
};
inline Step step(uint32_t file, uint32_t round, const alz_stream& s, bool sized) { return Step{file, round, s, sized, alz_result{0, 0, 0, 0}}; }
struct Checked { uint32_t file; uint64_t off; uint32_t len, want; };            // a frame's output and its content checksum word

// ---------------------------------------------------------------------------------------------- LZ4
// What the decode makes of lz4_replay's walk (alz_framing.h): the outcome of alz_container_decompress as far as the sizes tell it -- the
// decode of the last step confirms or replaces status and length -- with the file's steps, copies and checksummed frames appended.
struct Lz4Decode {
    uint32_t file; const alz_stream& fs; const uint8_t* src; const Lz4File& w;
    std::vector<Step>& steps; std::vector<alz_copy_range>& copies; std::vector<Checked>& checked;
    long last = -1;                                                             // the step that ends the file short of its last block
    const Lz4Frame* frame = nullptr; bool linked = false; uint32_t rounds = 0;  // rounds: what the compressed blocks of this frame in front of a block take

    int block(const Lz4Frame& f, const Lz4Block& b, uint64_t frame_start, uint64_t out, uint64_t room, const alz_result* m) {
        if (frame != &f) {
            // one LzWindows serves all blocks of a frame whatever its flag says (alz_container.cpp): a frame is linked when a block reaches back
            frame = &f; rounds = 0; linked = false;
            if (f.kind == Lz4Frame::FRAME)
                for (size_t i = 1; !linked && i < f.count; i++) { const Lz4Block& o = w.blocks[f.first + i]; linked = !o.raw && lz4_block_reaches_back(src + o.off, o.len); }
        }
        if (!m) {
            const uint64_t n = b.len > room ? room : b.len;
            if (n) copies.push_back(alz_copy_range{fs.src_off + b.off, fs.dst_off + out, (uint32_t)n, 0});
            return ALZ_OK;
        }
        const uint64_t hist = linked ? out - frame_start : 0;
        if (linked && (uint64_t)clamp32((size_t)room) + hist > 0xFFFFFF00ull) return ALZ_E_UNSUPPORTED;
        const bool sized = m->status == ALZ_ST_OK && m->dst_len <= room;
        // a block behind others of a linked frame waits for them only if it reads them
        const bool waits = linked && &b != w.blocks.data() + f.first && lz4_block_reaches_back(src + b.off, b.len);
        const uint32_t round = waits ? rounds : 0;
        rounds = round + 1 > rounds ? round + 1 : rounds;
        steps.push_back(step(file, round, body(ALZ_FMT_LZ4_BLOCK, fs.src_off + b.off, b.len, fs.dst_off + out, sized ? m->dst_len : clamp_cap(room), (uint32_t)hist), sized));
        return ALZ_OK;
    }
    size_t stopped(const Lz4Frame& f, const Lz4Block& b) { if (!b.raw) last = (long)steps.size() - 1; return f.end; }
    void content_checksum(uint64_t frame_start, uint64_t out, size_t pos) {
        checked.push_back(Checked{file, fs.dst_off + frame_start, (uint32_t)(out - frame_start), le32(src + pos)});
    }
};

// ---------------------------------------------------------------------------------------------- Snappy
struct SnappyFile {
    bool active = false, in_order = false;
    SnappyLayout lay; size_t first_step = 0;                                    // decode: the chunks at their declared places; their steps, in file order
    SnappyReader r = {10, 0, 0};                                                // in order / measure: the reader
    long wait_step = -1;                                                        // in order: the chunk that is out on the device
    size_t first = 0, count = 0;                                                // measure: this round's bodies in the batch
};
struct RangeSink {                                                              // a stored chunk is a range copy in HBM
    const alz_stream& fs; std::vector<alz_copy_range>& copies;
    void stored(size_t off, uint64_t out, uint32_t n) { copies.push_back(alz_copy_range{fs.src_off + off, fs.dst_off + out, n, 0}); }
};

// all chunks at their declared places, as snappy_file_decompress sends them out
void snappy_open(uint32_t file, const alz_stream& fs, const uint8_t* src, SnappyFile& w, alz_file_result& r, std::vector<Step>& steps, std::vector<alz_copy_range>& copies) {
    const size_t len = fs.src_len;
    if (!snappy_has_id(src, len)) { deliver(r, refused(ALZ_E_FORMAT)); return; }
    RangeSink sink{fs, copies};
    snappy_layout(src, len, fs.dst_cap, w.lay, sink);
    w.first_step = steps.size();
    for (const SnappyPiece& p : w.lay.pieces)
        if (!p.stored) steps.push_back(step(file, 0, body(ALZ_FMT_SNAPPY_RAW, fs.src_off + p.off, len - p.off, fs.dst_off + p.at, p.cap, 0), false));
    w.active = true;
}
// behind a round: the chunks of the first round are judged; a file that is read in order takes in the chunk that was out and sends the next
void snappy_advance(uint32_t file, uint32_t round, const alz_stream& fs, const uint8_t* src, SnappyFile& w, alz_file_result& r, std::vector<Step>& steps,
                    std::vector<alz_copy_range>& copies) {
    const size_t len = fs.src_len; const uint64_t cap = fs.dst_cap;
    Outcome o;
    if (!w.in_order) {
        if (snappy_judge(w.lay, cap, [&](size_t k) -> const alz_result& { return steps[w.first_step + k].got; }, w.r, o)) { w.active = false; deliver(r, o); return; }
        w.in_order = true;
    }
    const alz_result* got = w.wait_step >= 0 ? &steps[(size_t)w.wait_step].got : nullptr;
    w.wait_step = -1;
    RangeSink sink{fs, copies};
    if (snappy_read_on(src, len, cap, w.r, got, sink, o)) { w.active = false; deliver(r, o); return; }
    w.wait_step = (long)steps.size();
    steps.push_back(step(file, round, body(ALZ_FMT_SNAPPY_RAW, fs.src_off + w.r.pos, len - w.r.pos, fs.dst_off + w.r.out, clamp_cap(w.r.out < cap ? cap - w.r.out : 0), 0), false));
}

// one round of a measure: the bodies from the reader's position on, at the places their chunks declare
void snappy_collect(const alz_stream& fs, const uint8_t* src, SnappyFile& w, std::vector<alz_stream>& ss) {
    w.first = ss.size();
    snappy_measure_collect(src, fs.src_len, w.r.pos, [&](size_t off) { ss.push_back(body(ALZ_FMT_SNAPPY_RAW, fs.src_off + off, fs.src_len - off, 0, kNoBound, 0)); });
    w.count = ss.size() - w.first;
}

// ---------------------------------------------------------------------------------------------- the device side of a round
// the steps of round `round`, from step `from` on: one decode (alz_file_batch.h)
int run_round(alz_ctx* ctx, std::vector<Step>& steps, size_t from, uint32_t round, const void* d_src, void* d_dst) {
    std::vector<size_t> idx; std::vector<alz_stream> ss; std::vector<alz_result> rs; bool split;
    for (size_t k = from; k < steps.size(); k++) if (steps[k].round == round) { ss.push_back(steps[k].s); idx.push_back(k); }
    if (int e = run_long_and_short(ctx, ss, rs, d_src, d_dst, &split)) return e;
    for (size_t k = 0; k < idx.size(); k++) steps[idx[k]].got = rs[k];
    return ALZ_OK;
}

int measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, alz_file_result* results) {
    DeviceBuffer d_src(ctx);
    int rc;
    if ((rc = d_src.alloc(src_bytes)) || (src_bytes && (rc = alz_memcpy_h2d(ctx, d_src.p, src_base, src_bytes)))) return rc;
    std::vector<Lz4File> lz4(n); std::vector<size_t> lz4_first(n, 0); std::vector<SnappyFile> snappy(n);
    std::vector<alz_stream> ss; std::vector<alz_result> rs;
    uint32_t active = 0;
    for (uint32_t i = 0; i < n; i++) {
        results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
        const uint8_t* src = src_base + files[i].src_off;
        if (lz4_container(files[i].format)) {
            lz4_first[i] = ss.size();
            lz4_collect(src, files[i].src_len, lz4[i], [&](const Lz4Block& b) { ss.push_back(body(ALZ_FMT_LZ4_BLOCK, files[i].src_off + b.off, b.len, 0, kNoBound, 0)); });
        } else if (!snappy_has_id(src, files[i].src_len)) deliver(results[i], refused(ALZ_E_FORMAT));
        else { snappy[i].active = true; snappy_collect(files[i], src, snappy[i], ss); active++; }
    }
    for (bool first = true; first || active; first = false) {
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if (!ss.empty() && (rc = alz_measure_batch_device(ctx, nullptr, (uint32_t)ss.size(), (const uint8_t*)d_src.p, src_bytes, ss.data(), rs.data()))) return rc;
        for (uint32_t i = 0; i < n; i++) {
            const uint8_t* src = src_base + files[i].src_off;
            SnappyFile& w = snappy[i];
            if (first && lz4_container(files[i].format)) { Lz4Sizes sizes; deliver(results[i], lz4_replay(lz4[i], files[i].src_len, files[i].dst_cap, rs.data() + lz4_first[i], sizes)); }
            else if (w.active) {
                Outcome o;
                if (!snappy_measure_replay(src, files[i].src_len, files[i].dst_cap, w.r, files[i].src_off, ss.data() + w.first, w.count, rs.data() + w.first, o)) continue;
                if (o.rc == ALZ_E_INVALID) return o.rc;                         // (cannot happen: snappy_measure_replay)
                deliver(results[i], o); w.active = false; active--;
            }
        }
        ss.clear();
        for (uint32_t i = 0; i < n; i++) if (snappy[i].active) snappy_collect(files[i], src_base + files[i].src_off, snappy[i], ss);
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
        std::vector<alz_stream> ss; std::vector<alz_result> rs; std::vector<size_t> first(n, 0);
        for (uint32_t i = 0; i < n; i++) {
            if (!lz4_container(files[i].format)) continue;
            first[i] = ss.size();
            lz4_collect(src_base + files[i].src_off, files[i].src_len, lz4[i], [&](const Lz4Block& b) { ss.push_back(body(ALZ_FMT_LZ4_BLOCK, files[i].src_off + b.off, b.len, 0, kNoBound, 0)); });
        }
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if (!ss.empty() && (rc = alz_measure_batch_device(ctx, nullptr, (uint32_t)ss.size(), ds, src_bytes, ss.data(), rs.data()))) return rc;
        for (uint32_t i = 0; i < n; i++) {
            results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
            const uint8_t* src = src_base + files[i].src_off;
            if (lz4_container(files[i].format)) {
                Lz4Decode v{i, files[i], src, lz4[i], steps, copies, checked};
                deliver(results[i], lz4_replay(lz4[i], files[i].src_len, files[i].dst_cap, rs.data() + first[i], v));
                last[i] = v.last;
            } else snappy_open(i, files[i], src, snappy[i], results[i], steps, copies);
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
            if (!snappy[i].active) continue;
            snappy_advance(i, round + 1, files[i], src_base + files[i].src_off, snappy[i], results[i], steps, copies);
            if (!snappy[i].active) active--;
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
            if (sums[k] != checked[k].want && !redo[checked[k].file] && results[checked[k].file].rc != ALZ_E_CHECKSUM) deliver(results[checked[k].file], refused(ALZ_E_CHECKSUM));
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
        deliver(results[i], Outcome{frc, st, dl, su});
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
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, true, framed_container)) return rc;
    return n ? decode_batch(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results) : ALZ_OK;
}
int alz_framed_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                             alz_file_result* results) {
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, nullptr, 0, results, false, framed_container)) return rc;
    return n ? measure_batch(ctx, n, src_base, src_bytes, files, results) : ALZ_OK;
}
// files that alz_framed_decode_batch handed to the single-file layer because their decode did not confirm the measured sizes, process-wide
uint64_t alz_debug_framed_batch_refused(void) { return g_refused.load(std::memory_order_relaxed); }
// the host XXH32 the framing reader and the single-file layer use (alz_framing.h): what tools/bench_framed.py times next to the kernel
uint32_t alz_debug_host_xxh32(const uint8_t* p, size_t len, uint32_t seed) { return xxh32(p, len, seed); }

}   // extern "C"
