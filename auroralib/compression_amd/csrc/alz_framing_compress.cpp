// alz_framing_compress.cpp -- LZ4 (frame, legacy) and framed Snappy files WRITTEN in batches: alz_framing_compress_batch.  What
// alz_container_compress does for one such file, for a whole set in one call.  The contract is differential: per file the outcome and the
// bytes of the single-file call (alz_container.cpp), whose rules -- what is refused before encoding, descriptor, block words, stored or
// compressed, end marks, chunk headers, the order of the verdicts against the capacity -- are the writers of alz_framing.h, run here over
// another sink.  Pure host code on the public ABI plus the range-copy kernel (alz_xxh32.h).
//
// A single-file call encodes ONE file's blocks: a 64 KiB file is an encode batch of one stream, with two device allocations, an upload,
// a launch sequence and a download of its own.  Here the blocks of ALL files are one alz_encode_batch_device:
//   layout    every block of every file the writer does not refuse beforehand: 64 KiB chunks (Snappy), aux0 (frame), 8 MiB (legacy); its
//             compressed output goes to a slot of the size the single-file layer gives it
//   device    ONE allocation holds the uploaded source, the slots and a small table of header bytes.  One encode over all blocks (LZ4
//             blocks and raw Snappy chunks mix: one launch sequence per format); one alz_crc32c_batch_device over the raw bytes of all
//             Snappy chunks where they lie
//   settle    the writers of alz_framing.h run per file over the block results and the CRCs; their pieces -- header bytes, compressed
//             bodies out of the slots, stored bodies out of the source -- become ONE list of range copies from that allocation into the
//             file images, which come back through alz_file_batch::download
// A batch whose source and slots exceed a budget runs as consecutive groups of whole files, each group as above.
#include <atomic>
#include <chrono>
#include <cstring>
#include <vector>

#include "auroralz.h"
#include "alz_file_batch.h"
#include "alz_framing.h"
#include "alz_xxh32.h"

namespace {

using namespace alz_framing;
using namespace alz_file_batch;

const uint64_t kDefaultBudget = 2ull << 30;                                     // bytes of source + slots in one group
std::atomic<uint64_t> g_budget{kDefaultBudget};

enum { PH_LAYOUT, PH_UPLOAD, PH_ENCODE, PH_CRC, PH_SETTLE, PH_COPY, PH_DOWNLOAD, PH_COUNT };
double g_phase_ms[PH_COUNT];                                                    // of the last call, process-wide (alz_debug_framing_compress_phases)
struct PhaseClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(int ph) { const auto now = std::chrono::steady_clock::now(); g_phase_ms[ph] += std::chrono::duration<double, std::milli>(now - t).count(); t = now; }
};

inline bool lz4_container(uint32_t c) { return c == ALZ_C_LZ4_FRAME || c == ALZ_C_LZ4_LEGACY; }

// a file as the writer opened it: refused (rc), or `nb` blocks of `block` bytes from `first` on in the group's encode batch
struct Opened { int rc; Lz4Writer w; uint32_t block; size_t nb, first, first_crc; };

void open_file(const alz_stream& f, Opened& o) {
    o.nb = o.first = o.first_crc = 0;
    if (lz4_container(f.format)) { o.rc = lz4_write_open(f.format == ALZ_C_LZ4_LEGACY, f.aux0, f.src_len, f.dst_cap, o.w); o.block = o.w.block; }
    else { o.rc = snappy_write_open(f.dst_cap); o.block = kSnappyChunk; }
    if (o.rc == ALZ_OK) o.nb = ((size_t)f.src_len + o.block - 1) / o.block;
}
inline uint64_t slots_of(const Opened& o) { return (uint64_t)o.nb * write_slot_bytes(o.block); }
// header bytes a file can take in the table: magic / descriptor / stream identifier, a word or chunk header per block, the end mark
inline size_t table_bound(const Opened& o) { return 16 + o.nb * 8; }

// the sink of the batch (alz_framing.h): a piece is a range copy inside the device; header bytes travel through the table.  Neighbouring
// pieces that are neighbours at their origin too are one range.
struct BatchSink {
    std::vector<alz_copy_range>& copies; std::vector<uint8_t>& table;
    uint64_t table_at, src_at, img_at;                                          // the table and the file's source in the allocation; the file in the image buffer
    const alz_stream* blocks;                                                   // the file's streams of the encode batch
    void piece(uint64_t from, size_t at, size_t k) {
        if (!k) return;
        if (!copies.empty()) {
            alz_copy_range& l = copies.back();
            if (l.src_off + l.n == from && l.dst_off + l.n == img_at + at && (uint64_t)l.n + k <= 0x40000000u) { l.n += (uint32_t)k; return; }
        }
        copies.push_back(alz_copy_range{from, img_at + at, (uint32_t)k, 0});
    }
    void bytes(size_t at, const uint8_t* p, size_t k) { const size_t t = table.size(); table.insert(table.end(), p, p + k); piece(table_at + t, at, k); }
    void slot(size_t at, size_t i, size_t k) { piece(blocks[i].dst_off, at, k); }
    void source(size_t at, size_t off, size_t k) { piece(src_at + off, at, k); }
};

// files [g0, g1): one allocation, one encode, one CRC batch, one range copy, one download
int compress_group(alz_ctx* ctx, const alz_settings* settings, uint32_t g0, uint32_t g1, const uint8_t* src_base, const alz_stream* files,
                   uint8_t* dst_base, alz_file_result* results, std::vector<Opened>& opened) {
    PhaseClock clk;
    // ---- layout
    uint64_t lo = ~0ull, hi = 0, slots = 0; size_t nblk = 0, ncrc = 0, tbound = 0;
    for (uint32_t i = g0; i < g1; i++) {
        Opened& o = opened[i];
        results[i] = alz_file_result{o.rc, ALZ_ST_OK, 0, 0};
        if (o.rc != ALZ_OK) continue;
        tbound += table_bound(o);
        if (!o.nb) continue;
        lo = std::min<uint64_t>(lo, files[i].src_off); hi = std::max<uint64_t>(hi, files[i].src_off + files[i].src_len);
        o.first = nblk; nblk += o.nb; slots += slots_of(o);
        if (files[i].format == ALZ_C_SNAPPY) { o.first_crc = ncrc; ncrc += o.nb; }
    }
    if (nblk == 0) lo = hi = 0;
    if (nblk > 0x7FFFFFFFull) return ALZ_E_UNSUPPORTED;
    // [ pad | source lo .. hi | >= 64 bytes ][ slots ][ table ]: the source keeps its place modulo 256, and no block ends inside the last
    // 64 bytes of what the encoder is told is its source buffer
    const uint64_t pad = lo & 255u, src_al = (pad + (hi - lo) + 64 + 255) & ~255ull, table_at = src_al + slots, all = table_at + tbound;
    std::vector<alz_stream> ss(nblk), crc_ranges(ncrc);
    {
        uint64_t slot_at = src_al;
        for (uint32_t i = g0; i < g1; i++) {
            const Opened& o = opened[i];
            const size_t slot = write_slot_bytes(o.block);
            for (size_t k = 0; k < o.nb; k++) {
                alz_stream& s = ss[o.first + k]; memset(&s, 0, sizeof(s));
                const uint64_t off = (uint64_t)k * o.block;
                s.src_off = pad + (files[i].src_off - lo) + off; s.src_len = (uint32_t)std::min<uint64_t>(o.block, files[i].src_len - off);
                s.dst_off = slot_at; s.dst_cap = (uint32_t)slot; slot_at += slot;
                s.format = files[i].format == ALZ_C_SNAPPY ? ALZ_FMT_SNAPPY_RAW : ALZ_FMT_LZ4_BLOCK;
                if (files[i].format == ALZ_C_SNAPPY) crc_ranges[o.first_crc + k] = s;
            }
        }
    }
    clk.mark(PH_LAYOUT);
    // ---- device: source up, all blocks through one encode, all Snappy chunks through one CRC batch
    DeviceBuffer d_all(ctx), d_img(ctx);
    int rc;
    if ((rc = d_all.alloc((size_t)all))) return rc;
    uint8_t* da = (uint8_t*)d_all.p;
    if (hi > lo && (rc = alz_memcpy_h2d(ctx, da + pad, src_base + lo, (size_t)(hi - lo)))) return rc;
    clk.mark(PH_UPLOAD);
    std::vector<alz_result> rs(nblk); std::vector<uint32_t> crcs(ncrc);
    if (nblk && (rc = alz_encode_batch_device(ctx, nullptr, settings, (uint32_t)nblk, da, (size_t)src_al, ss.data(), da, (size_t)table_at, rs.data(), nullptr))) return rc;
    clk.mark(PH_ENCODE);
    if (ncrc && (rc = alz_crc32c_batch_device(ctx, (uint32_t)ncrc, da, (size_t)src_al, crc_ranges.data(), crcs.data()))) return rc;
    clk.mark(PH_CRC);
    // ---- settle: every file by its writer; a file that fails leaves no piece behind
    uint64_t dlo = ~0ull, dhi = 0;
    for (uint32_t i = g0; i < g1; i++) if (opened[i].rc == ALZ_OK) { dlo = std::min<uint64_t>(dlo, files[i].dst_off); dhi = std::max<uint64_t>(dhi, files[i].dst_off + files[i].dst_cap); }
    if (dhi <= dlo) return ALZ_OK;                                              // every file of the group was refused
    std::vector<alz_copy_range> copies; std::vector<uint8_t> table;
    table.reserve(tbound);
    for (uint32_t i = g0; i < g1; i++) {
        const Opened& o = opened[i];
        if (o.rc != ALZ_OK) continue;
        const size_t c0 = copies.size(), t0 = table.size();
        BatchSink sink{copies, table, table_at, o.nb ? ss[o.first].src_off : 0, files[i].dst_off - dlo, ss.data() + o.first};
        size_t len = 0;
        const alz_result* r = rs.data() + o.first;
        if (lz4_container(files[i].format)) rc = lz4_write_blocks(o.w, files[i].src_len, r, files[i].dst_cap, sink, &len);
        else rc = snappy_write_chunks(files[i].src_len, r, files[i].dst_cap, sink, [&](size_t k) { return crcs[o.first_crc + k]; }, &len);
        if (rc != ALZ_OK) { copies.resize(c0); table.resize(t0); results[i].rc = rc; continue; }
        results[i].dst_len = (uint32_t)len; results[i].src_used = files[i].src_len;
    }
    clk.mark(PH_SETTLE);
    // ---- the file images: assembled in HBM by one launch, downloaded once
    if (copies.empty()) return ALZ_OK;
    if (table.size() > tbound) return ALZ_E_INVALID;                            // (cannot happen: table_bound counts every piece a writer makes up)
    if ((rc = alz_memcpy_h2d(ctx, da + table_at, table.data(), table.size()))) return rc;
    if ((rc = d_img.alloc((size_t)(dhi - dlo)))) return rc;
    if ((rc = alz_host_range_copy(ctx, (uint32_t)copies.size(), copies.data(), da, (size_t)all, (uint8_t*)d_img.p, (size_t)(dhi - dlo)))) return rc;
    clk.mark(PH_COPY);
    std::vector<alz_stream> placed(files + g0, files + g1);
    for (alz_stream& f : placed) f.dst_off = f.dst_off >= dlo ? f.dst_off - dlo : 0;   // (a refused file may lie in front of dlo: it has no bytes)
    rc = download(ctx, g1 - g0, placed.data(), results + g0, d_img.p, dst_base + dlo);
    clk.mark(PH_DOWNLOAD);
    return rc;
}

}   // namespace

extern "C" {

int alz_framing_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                               const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, true, [](uint32_t c) { return lz4_container(c) || c == ALZ_C_SNAPPY; })) return rc;
    for (double& ms : g_phase_ms) ms = 0;
    if (n == 0) return ALZ_OK;
    std::vector<Opened> opened(n);
    for (uint32_t i = 0; i < n; i++) open_file(files[i], opened[i]);
    // consecutive groups of whole files: what a group uploads (the span of its sources) plus its slots stays within the budget, unless
    // one file alone exceeds it
    const uint64_t budget = g_budget.load(std::memory_order_relaxed);
    for (uint32_t g0 = 0; g0 < n;) {
        uint64_t lo = ~0ull, hi = 0, slots = 0; uint32_t g1 = g0;
        for (; g1 < n; g1++) {
            const Opened& o = opened[g1];
            if (o.nb) {
                const uint64_t nlo = std::min<uint64_t>(lo, files[g1].src_off), nhi = std::max<uint64_t>(hi, files[g1].src_off + files[g1].src_len);
                if (g1 > g0 && nhi - nlo + slots + slots_of(o) > budget) break;
                lo = nlo; hi = nhi; slots += slots_of(o);
            }
        }
        if (int rc = compress_group(ctx, settings, g0, g1, src_base, files, dst_base, results, opened)) return rc;
        g0 = g1;
    }
    return ALZ_OK;
}
// bytes of source plus slots that one group of alz_framing_compress_batch may hold on the device, for every context (ctx names the
// caller and must not be NULL); 0 restores the default of 2 GiB.  What the tests reach the grouping with at small sizes.
int alz_debug_framing_compress_budget(alz_ctx* ctx, uint64_t bytes) {
    if (!ctx) return ALZ_E_INVALID;
    g_budget.store(bytes ? bytes : kDefaultBudget, std::memory_order_relaxed);
    return ALZ_OK;
}
uint64_t alz_debug_framing_compress_budget_get(void) { return g_budget.load(std::memory_order_relaxed); }
// host milliseconds of the last alz_framing_compress_batch per phase, summed over its groups: layout, upload, encode, CRC-32C, settle,
// range copy, download.  Writes the first min(n, 7) and returns 7.  Process-wide: for a timing tool, not for concurrent callers.
int alz_debug_framing_compress_phases(double* out, int n) {
    if (!out || n < 0) return ALZ_E_INVALID;
    for (int i = 0; i < n && i < PH_COUNT; i++) out[i] = g_phase_ms[i];
    return PH_COUNT;
}

}   // extern "C"
