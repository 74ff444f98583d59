// alz_host.cpp -- context / plan management and the batch entry points of include/auroralz.h.
// Compiled by hipcc as host code; everything that computes runs in alz_kernels.hip.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <functional>
#include <thread>
#include <vector>
#include <sched.h>

#include "alz_internal.h"
#include "alz_measure.h"
#include "alz_rlh.h"
#include "alz_aplib.h"
#include "alz_inflate.h"
#include "alz_checksum.h"
#include "alz_xxh32.h"
#include "alz_bitlz.h"

static thread_local char g_err[512] = "";

// ALZ_TIMING=1: phase times of the host-buffer entry points on stderr (a tuning aid)
#include <chrono>
struct phase_timer {
    bool on; const char* what; std::chrono::steady_clock::time_point t;
    explicit phase_timer(const char* w) : on(getenv("ALZ_TIMING") != nullptr), what(w), t(std::chrono::steady_clock::now()) {}
    void mark(const char* phase) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[alz timing] %s: %s %.3f ms\n", what, phase, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// Host copies between the caller's (pageable) buffers and the pinned staging buffers run on a few threads: one core moves
// ~10 GB/s, a PCIe 5 x16 link ~55 GB/s, so a single memcpy loop left the link idle three quarters of the time.  One pool per
// context (the multi-GPU entry points drive one context per device from their own threads).  ALZ_COPY_THREADS overrides the
// thread count (1 = copy inline).
struct copy_job { uint8_t* dst; const uint8_t* src; size_t len; };
class copy_pool {
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv, done_cv;
    const copy_job* jobs = nullptr; size_t njobs = 0;
    std::atomic<size_t> next{0};
    size_t pending = 0; uint64_t gen = 0; bool stop = false;
    void work() { for (size_t i; (i = next.fetch_add(1, std::memory_order_relaxed)) < njobs;) memcpy(jobs[i].dst, jobs[i].src, jobs[i].len); }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return stop || gen != seen; }); if (stop) return; seen = gen; }
            work();
            { std::lock_guard<std::mutex> l(m); if (--pending == 0) done_cv.notify_one(); }
        }
    }
public:
    static int default_threads() {
        if (const char* e = getenv("ALZ_COPY_THREADS")) { const int v = atoi(e); return v < 1 ? 1 : (v > 64 ? 64 : v); }
        cpu_set_t set; int n = 1;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
        n /= 2;
        return n < 1 ? 1 : (n > 16 ? 16 : n);
    }
    explicit copy_pool(int nthreads) { for (int i = 1; i < nthreads; i++) th.emplace_back([this] { loop(); }); }
    ~copy_pool() {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv.notify_all();
        for (std::thread& t : th) t.join();
    }
    // runs every job; returns when all are done (the calling thread takes its share)
    void run(const std::vector<copy_job>& v) {
        size_t bytes = 0;
        for (const copy_job& j : v) bytes += j.len;
        if (th.empty() || bytes < (1u << 20)) { for (const copy_job& j : v) memcpy(j.dst, j.src, j.len); return; }
        { std::lock_guard<std::mutex> l(m); jobs = v.data(); njobs = v.size(); next.store(0); pending = th.size(); gen++; }
        cv.notify_all();
        work();
        std::unique_lock<std::mutex> l(m);
        done_cv.wait(l, [&] { return pending == 0; });
    }
};
// one copy, cut into pieces the pool can spread
static void add_copy(std::vector<copy_job>& v, uint8_t* dst, const uint8_t* src, size_t len) {
    const size_t piece = 1u << 20;
    for (size_t o = 0; o < len; o += piece) v.push_back(copy_job{dst + o, src + o, len - o < piece ? len - o : piece});
}

static int fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                                  \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ALZ_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

struct alz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // grow-only staging for the host-buffer entry points
    void* d_src = nullptr; size_t d_src_cap = 0;
    void* d_dst = nullptr; size_t d_dst_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // fork/join resources for per-format kernels of a mixed batch (they are independent: run them concurrently)
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};    // side streams of a mixed launch (with the launch stream: four lanes = the runtime's four hardware queues)
    hipEvent_t fork = nullptr, join[4] = {nullptr, nullptr, nullptr, nullptr};
    float last_kernel_ms = 0.f;                // device time of the kernels of the last timed / encode call (HIP events on the launch stream)
    bool exact = false;                        // alz_ctx_set_exact_kernels: the exact one-token-at-a-time kernels instead of the lane-parallel ones
    int variant = 0;                           // alz_ctx_set_kernel_variant
    uint64_t big_enc_launches = 0;             // streams the whole-GPU ENCODE path has taken (alz_encode_big.h)
    uint64_t seg_enc_launches = 0;             // launches of the segmented parse + emit (alz_encode_seg.h)
    int scan_mode = 0;                         // alz_debug_scan_mode: the encoder's scan path (enc_scan_select_kernel) -- 0 its probe decides, 1 every eligible stream, 2 off
    uint32_t seg_max_streams = 0xFFFFFFFFu;    // alz_debug_seg_max_streams: ~0 the rule, 0 the path off, else that many buffers instead of the rule -- of THIS context
    uint64_t chunk_repeats = 0;                // executes alz_plan_results repeated without the work queue (a bounded spin ran out)
    uint32_t big_min = 24u << 10;              // (24 KiB: tools/single_decode_sizes.py -- 0.18 ms either way at 16 KiB, 0.18 against 0.30 at 32) a lone stream of at least this many output bytes goes to the whole-GPU path (alz_big.hip)
    uint64_t big_launches = 0;                 // how often that path was enqueued
    uint32_t* d_big_accepted = nullptr;        // device words: [0] streams that path has ACCEPTED -- decoded itself, gate left closed (big_write bumps it; alz_ctx_big_stream reports it); [1] streams the encoder's scan path has taken
    hipEvent_t big_evt = nullptr; bool big_evt_set = false;   // behind the last whole-GPU decode that used d_bigbuf (plans that borrow it run one after the other)
    void* d_bigbuf = nullptr; size_t d_bigbuf_cap = 0;   // its scratch for the plans of the host-buffer entry points (grow-only)
    // two pinned staging buffers: host-buffer calls move the caller's (pageable) bytes through them, so that the memcpy of
    // one piece overlaps the PCIe transfer of the other
    void* pin[2] = {nullptr, nullptr}; size_t pin_cap = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};                     // pin_ev[k] was recorded behind a DMA on pin[k] and nobody has waited for it yet
    // grow-only scratch of download_packed (item table + dense copy)
    void* d_items = nullptr; size_t d_items_cap = 0;
    void* d_pack = nullptr; size_t d_pack_cap = 0;
    void* d_plan = nullptr; size_t d_plan_cap = 0;   // plan arrays of the host-buffer entry points (no hipMalloc / hipFree per call)
    // encoder scratch (prev links, narrowed links, matches, masks ...: ~45 GB for 10 000 x 256 KiB at quality 8), one grow-only slot
    // per purpose: allocating and freeing it per call cost 1-2 s, four times the kernels.  alz_ctx_release_scratch() returns it.
    enum { ENC_STREAMS, ENC_RESULTS, ENC_AUX, ENC_INDEX, ENC_POS, ENC_PREV4, ENC_PREVM, ENC_MATCH, ENC_SIDE, ENC_MASK, ENC_TAIL, ENC_BIG, ENC_SEL, ENC_NARROW, ENC_SEG, ENC_DEFLATE, ENC_REV, ENC_SLOTS };
    void* enc_buf[ENC_SLOTS] = {nullptr}; size_t enc_cap[ENC_SLOTS] = {0};
    copy_pool* pool = nullptr;                 // created with the pinned buffers
    std::vector<copy_job> jobs;                // (scratch of the staging loops)
    void copy(uint8_t* dst, const uint8_t* src, size_t len) { jobs.clear(); add_copy(jobs, dst, src, len); pool->run(jobs); }
};

static const size_t kPinBytes = 32u << 20;
#define ALZ_BIG_MAX_STREAMS 32u             /* a batch of at most this many streams, all of them big, may take the whole-GPU path stream by stream (plan_create weighs it) */

struct alz_plan {
    uint32_t n = 0;
    alz_lz_properties lz{};
    alz_stream* d_streams = nullptr;
    alz_result* d_results = nullptr;
    uint32_t* d_index = nullptr;            // concatenated per-format index lists
    uint32_t fmt_off[ALZ_FMT_COUNT] = {0};
    uint32_t fmt_cnt[ALZ_FMT_COUNT] = {0};
    bool borrowed = false;                  // the three device arrays live in the context's plan scratch (host-buffer entry points)
    std::vector<uint32_t> index_host;       // such a plan keeps its index list: its upload is not waited for (plan_create)
    // ONE big Yay0 / MIO0 stream: decoded by the whole GPU (alz_big.hip), the production kernel behind it only if that path declines
    // (or a few of them, one after the other: n streams through that path take n x ~0.1-0.3 ms, on wavefronts of their own they take as
    // long as the largest of them alone, 1-5 ms per MiB; plan_create weighs the two)
    bool big = false, big_borrowed = false; std::vector<alz_stream> big_streams; std::vector<uint32_t> big_pos; void* d_big = nullptr; uint32_t* d_gate = nullptr;
    // A big plan owns MUTABLE device state (val / jump / ctl / gate in d_big): two executes in flight on different streams would race on it.
    // Every execute waits for the event the one before recorded (the context's event when the scratch is the context's: several plans share it).
    hipEvent_t big_evt = nullptr; bool big_evt_set = false;
    // the stream of the last execute + an event behind it: alz_plan_results orders its copy behind the caller's own stream too
    hipEvent_t done_evt = nullptr; bool done_evt_set = false;
    // The flag-byte family as a work queue of (stream, chunk) items (alz_decode_fastq_kernel): for a format whose streams are more than the GPU holds
    // wavefronts, so that the launch does not end in a partly filled round.  One allocation: [64 control words | a 128-byte line per slot's flag | items | slots].
    struct chunk_plan { uint32_t n_items = 0, n_slots = 0, lw = 0; void* d_mem = nullptr; uint32_t* d_ctl = nullptr; uint32_t* d_flags = nullptr;
                        alz_chunk_item* d_items = nullptr; uint8_t* d_slots = nullptr; size_t zero_bytes = 0; alz_queue_bounds bounds{}; };
    chunk_plan chunk[ALZ_FMT_COUNT];
    // A queue plan owns MUTABLE device state too (queue heads, flags, hand-over slots): its executes are ordered one behind the other by `q_evt`, on whatever streams
    // the caller enqueues them (round 6; big plans: `big_evt`).  `d_tmo`: one STICKY word per format outside the region an execute zeroes -- a bounded spin that ran out
    // sets it, the gated launch enqueued behind every queue launch then decodes that format again with one wavefront per stream IN STREAM ORDER (so every execute is
    // whole when its stream gets past it, whichever buffers it ran on), nothing ever clears it, and alz_plan_results, seeing it, moves the plan off the queue for good.
    uint32_t* d_tmo = nullptr;
    hipEvent_t q_evt = nullptr; bool q_evt_set = false;     // q_evt_set: the event stands behind the last execute on a stream of the CALLER's
    bool q_ctx_pending = false;              // an execute went onto the context's own stream since: ordered by that stream itself, its event is recorded only when another stream needs it
    uint32_t epoch = 0;                      // of the last queue launch (1 .. 2^30 - 1; flags and heads are zeroed once, at creation, and again when the counter wraps)
    bool no_chunks = false;                  // a bounded spin of the queue kernel ran out once: this plan stays with the one-wavefront-per-stream kernels
};

static alz_lz_properties effective_lz(const alz_lz_properties* p) {
    alz_lz_properties lz;
    if (!p || p->window_bits == 0) {           // LZSS.DefaultProperties = LzProperties((byte)12, 4, 2)  LZSS.cs:33
        memset(&lz, 0, sizeof(lz)); lz.window_bits = 12; lz.length_bits = 4; lz.min_length = 3; lz.max_distance = 4096; lz.windows_start = 0xFEE;
    } else { lz = *p; if (lz.max_distance == 0) lz.max_distance = 1u << lz.window_bits; }
    return lz;
}

// ---------------------------------------------------------------- the rules the entry points share, each written once
// off + len <= total without wrapping (offsets are caller-supplied 64-bit values)
static inline bool range_ok(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }
// the LZSS geometries the GPU kernels take (the encoder asks for max_distance == 1 << window_bits on top)
static inline bool lzss_on_gpu(const alz_lz_properties& lz) { return lz.window_bits >= 8 && lz.window_bits <= 16 && lz.length_bits >= 1 && lz.length_bits <= 8; }
// an LZ4 block that continues a frame's window: its history, aux0 bytes in front of dst_off, would begin in front of the destination buffer
static inline bool lz4_history_outside(const alz_stream& s) { return s.format == ALZ_FMT_LZ4_BLOCK && s.aux0 > s.dst_off; }
static int refuse_lz4_history(uint32_t i, const alz_stream& s) {   // (the plan's wording: alz_plan_create, alz_decode_batch_multi)
    return lz4_history_outside(s) ? fail(ALZ_E_INVALID, "stream %u: history %u exceeds dst_off", i, s.aux0) : ALZ_OK;
}
static int no_refusal(uint32_t, const alz_stream&) { return ALZ_OK; }

// What a call is refused for, stream by stream, and per stream in this order: an unknown kind (`kinds` > 1: `format` must lie below it), a source
// range outside *src_bytes, a destination range outside *dst_bytes (NULL: the family has none), then the caller's own extra(i, stream) -> int.  `what`: the entry
// point's name in front of the batch families' texts, "" for the decoder, the encoder and the multi-GPU calls.  `ranges`: a table of byte ranges (the checksum families), with their wording.
template <class Extra>
static int validate_streams(const char* what, uint32_t kinds, uint32_t n, const alz_stream* streams, const size_t* src_bytes, const size_t* dst_bytes, Extra extra, bool ranges = false) {
    const char* sep = *what ? ": " : "";
    for (uint32_t i = 0; i < n; i++) {
        const alz_stream& s = streams[i];
        if (kinds > 1 && s.format >= kinds) return *what ? fail(ALZ_E_INVALID, "%s: stream %u: unknown format / kind %u", what, i, s.format) : fail(ALZ_E_INVALID, "stream %u: unknown format %u", i, s.format);
        if (src_bytes && !range_ok(s.src_off, s.src_len, *src_bytes))
            return ranges ? fail(ALZ_E_INVALID, "%s: range %u exceeds src_bytes", what, i) : fail(ALZ_E_INVALID, "%s%sstream %u: source range exceeds src_bytes", what, sep, i);
        if (dst_bytes && !range_ok(s.dst_off, s.dst_cap, *dst_bytes)) return fail(ALZ_E_INVALID, "%s%sstream %u: destination range exceeds dst_bytes", what, sep, i);
        if (int rc = extra(i, s)) return rc;
    }
    return ALZ_OK;
}

// The streams of a batch grouped per kind: `index` lists the stream numbers kind after kind, a kind's streams in input order; off[k] / cnt[k] is
// where kind k's list starts and how many it holds.  With a cost(i) the costliest streams of a kind come first (equal costs in input order).
static const uint32_t kMaxKinds = ALZ_ENCFMT_END;   // (the encoder's slots: the public formats, FastLZ level 2, the two internal ones of alz_bitlz.h)
static_assert(ALZ_RLH_COUNT <= kMaxKinds && ALZ_BITLZ_COUNT <= kMaxKinds, "the per-kind counters of group_streams");
template <class KindOf>
static void group_streams(uint32_t n, uint32_t kinds, KindOf kind_of, std::vector<uint32_t>& index, uint32_t* off, uint32_t* cnt) {
    uint32_t fill[kMaxKinds] = {0};
    index.assign(n ? n : 1, 0u);
    for (uint32_t f = 0; f < kinds; f++) cnt[f] = 0;
    for (uint32_t i = 0; i < n; i++) cnt[kind_of(i)]++;
    for (uint32_t f = 0, at = 0; f < kinds; f++) { off[f] = at; at += cnt[f]; }
    for (uint32_t i = 0; i < n; i++) { const uint32_t f = kind_of(i); index[off[f] + fill[f]++] = i; }
}
template <class KindOf, class Cost>
static void group_streams(uint32_t n, uint32_t kinds, KindOf kind_of, Cost cost, std::vector<uint32_t>& index, uint32_t* off, uint32_t* cnt) {
    group_streams(n, kinds, kind_of, index, off, cnt);
    for (uint32_t f = 0; f < kinds; f++)
        if (cnt[f] > 1) std::stable_sort(index.begin() + off[f], index.begin() + off[f] + cnt[f], [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
}

// One timed run on the context's stream: uploads(), ev0, launches(), ev1, downloads() -- each -> hipError_t, each skipped once one has failed --
// and ALWAYS a wait for the stream before the return: the copies read and write the caller's tables and the caller's locals.  The first error is
// reported under `what`; the time between the two events becomes last_kernel_ms.
template <class Uploads, class Launches, class Downloads>
static int launch_bracket(alz_ctx* c, const char* what, Uploads uploads, Launches launches, Downloads downloads) {
    hipError_t e = uploads();
    if (e == hipSuccess) e = hipEventRecord(c->ev0, c->stream);
    if (e == hipSuccess) e = launches();
    if (e == hipSuccess) e = hipEventRecord(c->ev1, c->stream);
    if (e == hipSuccess) e = downloads();
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ALZ_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_kernel_ms = ms;
    return ALZ_OK;
}

// The context list of a multi-GPU call: no NULL, none twice
static int check_contexts(const char* what, alz_ctx* const* ctxs, uint32_t n_ctx) {
    for (uint32_t q = 0; q < n_ctx; q++) {
        if (!ctxs[q]) return fail(ALZ_E_INVALID, "%s: context %u is NULL", what, q);
        for (uint32_t r = 0; r < q; r++) if (ctxs[r] == ctxs[q]) return fail(ALZ_E_INVALID, "%s: context %u is listed twice (a context is single-threaded)", what, q);
    }
    return ALZ_OK;
}
// greedy LPT: longest job first onto the least loaded part (equal jobs, as in the metric's batches, are dealt round-robin); load[] starts at zero
template <class Cost>
static void lpt_deal(uint32_t n, uint32_t n_parts, Cost cost, uint32_t* part_of, uint64_t* load) {
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost(a) > cost(b); });
    for (uint32_t k = 0; k < n; k++) {
        uint32_t best = 0;
        for (uint32_t q = 1; q < n_parts; q++) if (load[q] < load[best]) best = q;
        part_of[order[k]] = best; load[best] += cost(order[k]);
    }
}
// A batch dealt out over contexts, part[i] the context of stream i: work(q, idx) -> int runs context q's share, idx its stream numbers (ascending:
// source order; an empty share is skipped).  One host thread per context (a context is single-threaded; distinct contexts run concurrently), no collective: the shares are
// independent.  The first share that failed is reported, with its thread's text.
template <class Work>
static int run_shares(alz_ctx* const* ctxs, uint32_t n_ctx, uint32_t n, const uint32_t* part, uint32_t* part_of_out, Work work) {
    if (part_of_out) for (uint32_t i = 0; i < n; i++) part_of_out[i] = part[i];
    std::vector<std::vector<uint32_t>> idx(n_ctx);
    for (uint32_t i = 0; i < n; i++) idx[part[i]].push_back(i);
    std::vector<int> rcs(n_ctx, ALZ_OK); std::vector<std::string> errs(n_ctx);
    auto run = [&](uint32_t q) { if (!idx[q].empty() && (rcs[q] = work(q, idx[q]))) errs[q] = g_err; };
    std::vector<std::thread> th;
    for (uint32_t q = 1; q < n_ctx; q++) th.emplace_back(run, q);
    run(0);
    for (std::thread& t : th) t.join();
    for (uint32_t q = 0; q < n_ctx; q++) if (rcs[q]) return fail(rcs[q], "context %u (device %d): %s", q, ctxs[q]->device, errs[q].c_str());
    return ALZ_OK;
}

extern "C" {

int alz_abi_version(void) { return ALZ_ABI_VERSION; }
int alz_ctx_big_stream(alz_ctx* c, uint32_t min_bytes, uint64_t* launches_out) {
    if (!c) return fail(ALZ_E_INVALID, "alz_ctx_big_stream: ctx is NULL");
    if (min_bytes) c->big_min = min_bytes;
    if (launches_out) {
        // streams the two whole-GPU paths have TAKEN: the decode side counts on the device, where the path decides (a stream it declines goes to the kernel behind the gate
        // and is not counted); everything enqueued so far on any stream is waited for, so the number is exact when the caller asks
        uint32_t acc = 0;
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        if (c->d_big_accepted) HIP_TRY(hipMemcpy(&acc, c->d_big_accepted, sizeof(acc), hipMemcpyDeviceToHost));
        *launches_out = (uint64_t)acc + c->big_enc_launches;
    }
    return ALZ_OK;
}
int alz_ctx_set_kernel_variant(alz_ctx* c, int variant) {
    if (!c || variant < 0 || variant > 3) return fail(ALZ_E_INVALID, "alz_ctx_set_kernel_variant: bad argument");
    c->variant = variant;
    return ALZ_OK;
}
int alz_ctx_set_exact_kernels(alz_ctx* c, int on) {
    if (!c) return fail(ALZ_E_INVALID, "ctx is NULL");
    c->exact = on != 0;
    return ALZ_OK;
}
/* not in the public header: resident waves per CU of the production kernel of `format` (tuning aid) */
int alz_debug_occupancy(int format) { return alz_kernel_occupancy(format); }
/* not in the public header: the largest batch (buffers of one format) whose parse + emit runs over segments (alz_encode_seg.h; 0: never), and how often a context has gone that way */
void alz_debug_seg_max_streams(alz_ctx* c, uint32_t v) { if (c) c->seg_max_streams = v; }
/* not in the public header: the encoder's scan path (streams whose parse visits few positions go without kernels A and B): 0 the probe decides, 1 every eligible stream, 2 off */
void alz_debug_scan_mode(alz_ctx* c, int mode) { if (c && mode >= 0 && mode <= 2) c->scan_mode = mode; }
/* ... and how many streams have gone that way on this context (counted on the device, where the probe decides; waits for the device) */
uint64_t alz_debug_scan_streams(alz_ctx* c) {
    uint32_t v = 0;
    if (!c || !c->d_big_accepted || hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(&v, c->d_big_accepted + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return v;
}
uint64_t alz_debug_seg_launches(const alz_ctx* c) { return c ? c->seg_enc_launches : 0; }
/* not in the public header: which kernel B each stream of the LAST encode launch went to -- the first n words of the ENC_SEL scratch, enc_probe_kernel's word per stream
   (bit 0: the one-position-per-lane kernel, bits 8 and up: hits per thousand sampled positions).  Meaningful behind a call of ONE format whose finder has the probe
   (maxChain >= 3, 16-bit links, one property set); waits for the device.  Returns the words copied, -1 without that scratch. */
int alz_debug_enc_probe_words(alz_ctx* c, uint32_t* out, uint32_t n) {
    if (!c || !out || !c->enc_buf[alz_ctx::ENC_SEL] || c->enc_cap[alz_ctx::ENC_SEL] < (size_t)n * sizeof(uint32_t)) return -1;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, c->enc_buf[alz_ctx::ENC_SEL], (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)n;
}
/* not in the public header: how often alz_plan_results has repeated a launch without the work queue on this context (expected: never) */
uint64_t alz_debug_chunk_repeats(const alz_ctx* c) { return c ? c->chunk_repeats : 0; }
/* not in the public header: output bytes per chunk of the work-queue kernels */
int alz_debug_chunk_bytes(void) { return (int)ALZ_CHUNK_OUT; }
/* not in the public header: the (stream, chunk) items of a plan's work queues (0: the plan decodes with one wavefront per stream) */
/* not in the public header: the control words of a format's work queue (256 (e & 1) + 32 q, q < 8: the head of sub-queue q in the set launch e drew from = tickets drawn; word 1: the plan's sticky
   timeout word for the format, which lives elsewhere and is shown here) and, behind them from word ALZ_CHUNK_CTL_WORDS = 512 on, the flag of every hand-over slot (one per 32 words), reduced to the
   state the LAST launch left */
int alz_debug_plan_queue_ctl(alz_plan* p, int fmt, uint32_t* out, uint32_t nwords) {
    if (!p || fmt < 0 || fmt >= ALZ_FMT_COUNT || !p->chunk[fmt].d_ctl) return -1;
    const uint32_t have = ALZ_CHUNK_CTL_WORDS + p->chunk[fmt].n_slots * ALZ_CHUNK_FLAG_STRIDE;
    if (nwords > have) nwords = have;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, p->chunk[fmt].d_ctl, 4 * (size_t)nwords, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (uint32_t k = ALZ_CHUNK_CTL_WORDS; k < nwords; k += ALZ_CHUNK_FLAG_STRIDE) out[k] = (out[k] >> 2) == p->epoch ? (out[k] & 3u) : 0u;   // (flags of the LAST launch: 0 not set, 1 handed over, 2 ended, 3 timed out)
    if (nwords > 1u && p->d_tmo && hipMemcpy(out + 1, p->d_tmo + fmt, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)nwords;
}
int alz_debug_plan_queue_items(alz_plan* p) { int n = 0; if (p) for (int f = 0; f < ALZ_FMT_COUNT; f++) n += (int)p->chunk[f].n_items; return n; }
const char* alz_last_error(void) { return g_err; }

int alz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int alz_create(int device, alz_ctx** out) {
    if (!out) return fail(ALZ_E_INVALID, "alz_create: out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(ALZ_E_NO_DEVICE, "no HIP device: the auroralz ABI has no CPU fallback");
    if (device < 0 || device >= n) return fail(ALZ_E_INVALID, "device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    alz_ctx* c = new (std::nothrow) alz_ctx();
    if (!c) return fail(ALZ_E_NOMEM, "out of host memory");
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming);
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&c->join[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_big_accepted, 256);
    if (e == hipSuccess) e = hipMemset(c->d_big_accepted, 0, 256);
    if (e != hipSuccess) { alz_destroy(c); return fail(ALZ_E_HIP, "context creation failed: %s", hipGetErrorString(e)); }   // (what was created so far goes with it)
    *out = c;
    return ALZ_OK;
}

static void release_scratch(alz_ctx* c);
void alz_destroy(alz_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    release_scratch(c);
    for (int i = 0; i < 2; i++) { if (c->pin[i]) (void)hipHostFree(c->pin[i]); if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]); }
    if (c->big_evt) (void)hipEventDestroy(c->big_evt);
    if (c->d_big_accepted) (void)hipFree(c->d_big_accepted);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->fork) (void)hipEventDestroy(c->fork);
    for (int i = 0; i < 4; i++) if (c->join[i]) (void)hipEventDestroy(c->join[i]);
    for (int i = 0; i < 3; i++) if (c->aux[i]) (void)hipStreamDestroy(c->aux[i]);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c->pool;
    delete c;
}

int alz_device_info(alz_ctx* c, char* name, size_t name_cap, int* cu_count, uint64_t* hbm_bytes) {
    if (!c) return fail(ALZ_E_INVALID, "ctx is NULL");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, c->device));
    if (name && name_cap) { snprintf(name, name_cap, "%s (%s)", p.name, p.gcnArchName); }
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (uint64_t)p.totalGlobalMem;
    return ALZ_OK;
}

// ---------------------------------------------------------------- device memory helpers
int alz_device_malloc(alz_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(d_ptr, bytes + 64));              // (+ the read slack of the device-resident entry points, auroralz.h)
    return ALZ_OK;
}
int alz_device_free(alz_ctx* c, void* d_ptr) {
    if (!c) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipFree(d_ptr));
    return ALZ_OK;
}
static int staged_h2d(alz_ctx* c, void* d_dst, const uint8_t* h_src, size_t bytes);
static int staged_d2h(alz_ctx* c, uint8_t* h_dst, const void* d_src, size_t bytes);
int alz_memcpy_h2d(alz_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
    if (!c) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = staged_h2d(c, d_dst, (const uint8_t*)h_src, bytes)) return rc;      // (pageable memory: through the pinned buffers + copy threads)
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALZ_OK;
}
int alz_memcpy_d2h(alz_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
    if (!c) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = staged_d2h(c, (uint8_t*)h_dst, d_src, bytes)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALZ_OK;
}
int alz_memset_d(alz_ctx* c, void* d_dst, int value, size_t bytes) {
    if (!c) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(d_dst, value, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALZ_OK;
}
int alz_synchronize(alz_ctx* c) {
    if (!c) return fail(ALZ_E_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ALZ_OK;
}

// ---------------------------------------------------------------- plans
void alz_plan_destroy(alz_ctx* c, alz_plan* p) {
    if (!p) return;
    if (c) (void)hipSetDevice(c->device);
    if (!p->borrowed) {
        if (p->d_streams) (void)hipFree(p->d_streams);
        if (p->d_results) (void)hipFree(p->d_results);
        if (p->d_index) (void)hipFree(p->d_index);
    }
    if (p->d_big && !p->big_borrowed) (void)hipFree(p->d_big);
    if (p->big_evt) (void)hipEventDestroy(p->big_evt);
    if (p->q_evt) (void)hipEventDestroy(p->q_evt);
    if (p->d_tmo) (void)hipFree(p->d_tmo);
    if (p->done_evt) (void)hipEventDestroy(p->done_evt);
    for (int f = 0; f < ALZ_FMT_COUNT; f++) if (p->chunk[f].d_mem) (void)hipFree(p->chunk[f].d_mem);
    delete p;
}

static int grow(alz_ctx* c, void** buf, size_t* cap, size_t need);
// The three device tables of a batch of n streams -- streams | results | index, the first two rounded up to 256 bytes -- out of the context's
// grow-only plan scratch, which one batch at a time uses
struct plan_tables { alz_stream* streams; alz_result* results; uint32_t* index; };
static int carve_plan_scratch(alz_ctx* c, size_t n, plan_tables* t) {
    const size_t a = (n * sizeof(alz_stream) + 255) & ~(size_t)255, b = (n * sizeof(alz_result) + 255) & ~(size_t)255;
    if (int rc = grow(c, &c->d_plan, &c->d_plan_cap, a + b + n * sizeof(uint32_t))) return rc;
    t->streams = (alz_stream*)c->d_plan; t->results = (alz_result*)((uint8_t*)c->d_plan + a); t->index = (uint32_t*)((uint8_t*)c->d_plan + a + b);
    return ALZ_OK;
}
// `scratch`: the plan's device arrays come out of the context's grow-only plan scratch (one plan at a time: the host-buffer
// entry points, which create, run and drop a plan inside one call -- a hipMalloc / hipFree trio per call cost more than the
// kernel of a small batch)
static int plan_create(alz_ctx* c, const alz_lz_properties* props, uint32_t n, const alz_stream* streams, alz_plan** out, bool scratch) {
    if (!c || !out || (n && !streams)) return fail(ALZ_E_INVALID, "alz_plan_create: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    alz_lz_properties lz = effective_lz(props);
    if (int rc = validate_streams("", ALZ_FMT_COUNT, n, streams, nullptr, nullptr, [](uint32_t i, const alz_stream& s) -> int {   // (no buffer sizes here: no ranges)
            if (int rc = refuse_lz4_history(i, s)) return rc;
            if (s.format == ALZ_FMT_LZ4_BLOCK && s.aux0 && (uint64_t)s.aux0 + s.dst_cap > 0xFFFFFF00ull) return fail(ALZ_E_UNSUPPORTED, "stream %u: history + dst_cap exceed 4 GiB", i);
            return ALZ_OK;
        })) return rc;
    // Longest first inside a format's launch: workgroups are dispatched in index order and a CU holds ~24 of them, so the
    // costly streams start at once and the cheap ones fill the tail.  A stream's cost is its tokens (~ compressed bytes)
    // plus its output bytes: the 256 KiB windows of Test.bmp take 2.8 ms (flat, ratio 0.02) to 9.2 ms (photographic, ratio
    // 0.59) per 10 000; in input order that batch ran 5.8 ms per launch (tools/realistic_windows.py).
    uint32_t cnt[ALZ_FMT_COUNT], off[ALZ_FMT_COUNT]; std::vector<uint32_t> index;
    group_streams(n, ALZ_FMT_COUNT, [&](uint32_t i) { return streams[i].format; },
                  [&](uint32_t i) { return 3ull * streams[i].src_len + (streams[i].decom_len ? streams[i].decom_len : streams[i].dst_cap); }, index, off, cnt);
    if (cnt[ALZ_FMT_LZSS] && !lzss_on_gpu(lz)) return fail(ALZ_E_UNSUPPORTED, "LZSS geometry outside the GPU path (window_bits 8..16, length_bits 1..8)");
    alz_plan* p = new (std::nothrow) alz_plan();
    if (!p) return fail(ALZ_E_NOMEM, "out of host memory");
    p->n = n; p->lz = lz;
    memcpy(p->fmt_off, off, sizeof(off)); memcpy(p->fmt_cnt, cnt, sizeof(cnt));
    size_t nn = n ? n : 1;
    hipError_t e = hipSuccess;
    if (scratch) {
        plan_tables t;
        if (int rc = carve_plan_scratch(c, nn, &t)) { delete p; return rc; }
        p->borrowed = true;
        p->d_streams = t.streams; p->d_results = t.results; p->d_index = t.index;
    } else {
        e = hipMalloc((void**)&p->d_streams, nn * sizeof(alz_stream));
        if (e == hipSuccess) e = hipMalloc((void**)&p->d_results, nn * sizeof(alz_result));
        if (e == hipSuccess) e = hipMalloc((void**)&p->d_index, nn * sizeof(uint32_t));
    }
    if (e == hipSuccess && n) e = hipMemcpyAsync(p->d_streams, streams, n * sizeof(alz_stream), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n) e = hipMemcpyAsync(p->d_index, index.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(p->d_results, 0xFF, nn * sizeof(alz_result), c->stream);
    // (a plan of the library's own -- one host-buffer call: created, executed, read, destroyed -- does not wait here: the caller's stream
    // table outlives the call, the index list moves into the plan, and the kernels queue up behind the uploads; the one stream of a
    // format class's Decompress call pays ~30 us for every synchronisation)
    if (scratch) p->index_host = std::move(index);
    else if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); alz_plan_destroy(c, p); return fail(ALZ_E_HIP, "plan upload failed: %s", hipGetErrorString(e)); }
    bool all_big = n >= 1 && n <= ALZ_BIG_MAX_STREAMS && !c->exact && c->variant == 0;
    for (uint32_t i = 0; all_big && i < n; i++) all_big = alz_big_eligible((int)streams[i].format, &streams[i], &lz, c->big_min);
    if (all_big && n > 1) {
        // several big streams: one after the other through the whole-GPU path (measured: ~0.08 ms of launches + 0.1 ms per MiB of output
        // each) against all of them side by side on wavefronts of their own, which takes as long as the LARGEST of them alone (~4.4 ms per
        // MiB): 16 streams of 1 MiB 2.9 against 4.4 ms, 32 streams of 256 KiB 3.4 against 1.1
        double t_big = 0, t_lone = 0;
        for (uint32_t i = 0; i < n; i++) {
            const double mib = (double)(streams[i].decom_len ? streams[i].decom_len : streams[i].dst_cap) / 1048576.0;
            t_big += 0.08 + 0.1 * mib;
            if (4.4 * mib > t_lone) t_lone = 4.4 * mib;
        }
        all_big = t_big < t_lone;
    }
    if (all_big) {
        // (the scratch -- 4 bytes per output byte of the largest stream, they run one after the other -- belongs to the plan; when it cannot
        // be had the production kernels decode the streams)
        size_t need = 0;
        for (uint32_t i = 0; i < n; i++) { const size_t b = alz_big_scratch_bytes((int)streams[i].format, &streams[i]) + 64; if (b > need) need = b; }
        if (scratch) { if (grow(c, &c->d_bigbuf, &c->d_bigbuf_cap, need) == ALZ_OK) { p->d_big = c->d_bigbuf; p->big_borrowed = true; } }
        else if (hipMalloc(&p->d_big, need) != hipSuccess) { p->d_big = nullptr; (void)hipGetLastError(); }
        if (p->d_big) {
            p->big = true; p->big_streams.assign(streams, streams + n); p->d_gate = (uint32_t*)((uint8_t*)p->d_big + need - 64);
            p->big_pos.resize(n);
            const std::vector<uint32_t>& ix = scratch ? p->index_host : index;
            for (uint32_t k = 0; k < n; k++) p->big_pos[ix[k]] = k;      // where stream i sits in the (per-format, cost-ordered) index list
        }
    }
    // ---- the work queue of chunks (device-resident plans): a format whose streams are more than the GPU holds of its wavefronts, and
    // long enough to be cut.  Failing to get the memory only means the one-wavefront-per-stream launch.
    const bool force_queue = c->variant == 3;     // (plans created while the context is in variant 3 use the queue whatever the number of streams: the parity tests)
    if (!scratch && !c->exact && (force_queue || (!p->big && c->variant == 0))) {
        hipDeviceProp_t pr;
        const bool have_pr = hipGetDeviceProperties(&pr, c->device) == hipSuccess;
        for (int f = 0; f < ALZ_FMT_COUNT && have_pr; f++) {
            uint32_t lw = 0;
            if (!cnt[f] || !alz_chunk_format(f, &lz, &lw)) continue;
            const int occ = alz_chunk_places_per_cu(f);
            const uint32_t chb = alz_chunk_bytes(f);
            // (from 0.6 of the GPU's wavefront places on: 10 000 x 256 KiB as Yaz0, ms per launch one wavefront per stream / queue -- 3 000 streams 1.12 (two wavefronts each) / 1.33,
            // 4 000 1.44 / 1.40, 5 000 1.60 / 1.49, 6 400 2.43 / 1.69, 8 000 2.09 (queue); below that everything is resident at once and a stream's own latency decides)
            // -- counted per FORMAT: in a mixed batch the formats' kernels run side by side, and queues whose items wait for each other take the places the others need (the cfg4 shard, 5 000 mixed
            // streams: 2.54 ms with one wavefront per stream, 3.20 with its three flag-byte formats as queues)
            // PRS (two wavefronts per stream, bound by the scalar pipe: a stream in a half-empty GPU is fast anyway) only above what the GPU holds: 2 000 / 3 000 / 4 000 / 6 000 / 10 000 streams
            // 1.39 / 1.69 / 2.72 / 3.43 / 5.50 ms with a workgroup per stream, 1.59 / 1.80 / 2.34 / 3.32 / 5.36 as a queue (3 072 places)
            // (with 40 KiB chunks and the descriptor table -- 29 places per CU for Yaz0 / LZ11 -- the queue wins earlier: 3 600 / 4 200 streams 1.44 / 1.58 ms one wavefront per stream, 1.37 / 1.42 as a
            // queue: from 0.4 of the places on, and never where two wavefronts share a stream -- up to 3 072 streams: 3 000 streams 1.14 that way, 1.31 as a queue)
            const uint64_t tenths = (f == ALZ_FMT_PRS_BE || f == ALZ_FMT_PRS_LE) ? 10ull : 4ull;
            if (!force_queue && (occ < 1 || cnt[f] <= alz_two_wave_max() || 10ull * cnt[f] <= tenths * (uint64_t)occ * (uint64_t)pr.multiProcessorCount)) continue;
            // items in chunk-major order over the format's cost-ordered list; a stream's slots are consecutive
            std::vector<uint32_t> nch(cnt[f]), base(cnt[f]);
            uint32_t slots = 0, maxch = 0; uint64_t items64 = 0;
            for (uint32_t k = 0; k < cnt[f]; k++) {
                const alz_stream& st = streams[index[p->fmt_off[f] + k]];
                const uint32_t bound = st.decom_len ? (st.decom_len < st.dst_cap ? st.decom_len : st.dst_cap) : st.dst_cap;
                uint32_t m = (bound + chb - 1u) / chb; if (m == 0) m = 1;
                nch[k] = m; base[k] = slots; slots += m; items64 += m; if (m > maxch) maxch = m;
            }
            if (maxch < 2 || items64 > 0x3FFFFFFFull) continue;
            // ALZ_QUEUE_SHARDS sub-queues, one behind the other: stream k of the cost-ordered list goes to sub-queue k mod 8 (every sub-queue gets its share of the costly
            // streams, and the sub-queues come out equally long: workgroups are dealt round-robin over the XCDs and each prefers its XCD's sub-queue), chunk-major inside
            std::vector<alz_chunk_item> items; items.reserve((size_t)items64);
            alz_queue_bounds qb{};
            for (uint32_t q = 0; q < ALZ_QUEUE_SHARDS; q++) {
                qb.off[q] = (uint32_t)items.size();
                for (uint32_t ch = 0; ch < maxch; ch++)
                    for (uint32_t k = q; k < cnt[f]; k += ALZ_QUEUE_SHARDS)
                        if (ch < nch[k]) items.push_back(alz_chunk_item{index[p->fmt_off[f] + k], ch, base[k] + ch, ch + 1u == nch[k] ? 1u : 0u});
            }
            qb.off[ALZ_QUEUE_SHARDS] = (uint32_t)items.size();
            alz_plan::chunk_plan& cp = p->chunk[f];
            const size_t zero_bytes = (4 * (size_t)ALZ_CHUNK_CTL_WORDS + (size_t)slots * 4 * ALZ_CHUNK_FLAG_STRIDE + 255) & ~(size_t)255, items_bytes = (items.size() * sizeof(alz_chunk_item) + 255) & ~(size_t)255;
            const size_t slot_bytes = (size_t)slots * (32 + lw);
            if (hipMalloc(&cp.d_mem, zero_bytes + items_bytes + slot_bytes + 256) != hipSuccess) { cp.d_mem = nullptr; (void)hipGetLastError(); continue; }
            cp.d_ctl = (uint32_t*)cp.d_mem; cp.d_flags = cp.d_ctl + ALZ_CHUNK_CTL_WORDS; cp.zero_bytes = zero_bytes; cp.bounds = qb;
            cp.d_items = (alz_chunk_item*)((uint8_t*)cp.d_mem + zero_bytes); cp.d_slots = (uint8_t*)cp.d_mem + zero_bytes + items_bytes;
            if (hipMemset(cp.d_mem, 0, zero_bytes) != hipSuccess || hipMemcpy(cp.d_items, items.data(), items.size() * sizeof(alz_chunk_item), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(cp.d_mem); cp = alz_plan::chunk_plan(); (void)hipGetLastError(); continue; }
            cp.n_items = (uint32_t)items.size(); cp.n_slots = slots; cp.lw = lw;
            if (!p->d_tmo) {                                   // the sticky timeout words, one per format (zeroed ONCE, here)
                if (hipMalloc((void**)&p->d_tmo, 256) != hipSuccess || hipMemset(p->d_tmo, 0, 256) != hipSuccess) {
                    if (p->d_tmo) (void)hipFree(p->d_tmo);
                    p->d_tmo = nullptr; (void)hipFree(cp.d_mem); cp = alz_plan::chunk_plan(); (void)hipGetLastError();
                }
            }
        }
    }
    *out = p;
    return ALZ_OK;
}
int alz_plan_create(alz_ctx* c, const alz_lz_properties* props, uint32_t n, const alz_stream* streams, alz_plan** out) {
    return plan_create(c, props, n, streams, out, false);
}

static uint32_t format_weight(uint32_t fmt);
// Time of ONE 256 KiB stream alone on the GPU, in units of 10 us (measured: docs/EXPERIMENTS.md 4.4 / 8): what orders the kernels of a mixed launch
static uint32_t format_latency(uint32_t fmt) {
    switch (fmt) {
    case ALZ_FMT_YAY0: return 91;
    case ALZ_FMT_YAZ0: case ALZ_FMT_LZ11: case ALZ_FMT_LZ40: case ALZ_FMT_LZ02: case ALZ_FMT_PRS_BE: case ALZ_FMT_PRS_LE: return 109;
    case ALZ_FMT_MIO0: case ALZ_FMT_SMSR00: return 125;
    case ALZ_FMT_LZSS: case ALZ_FMT_LZ10: case ALZ_FMT_CLZ0: case ALZ_FMT_CNS: case ALZ_FMT_LZHUDSON: case ALZ_FMT_LZSHREK: return 154;
    case ALZ_FMT_LZ4_BLOCK: case ALZ_FMT_FASTLZ: case ALZ_FMT_WFLZ: case ALZ_FMT_WFLZ_BE: case ALZ_FMT_HIG: case ALZ_FMT_CNX2: return 170;
    case ALZ_FMT_BLZ: case ALZ_FMT_REFPACK: case ALZ_FMT_SNAPPY_RAW: return 200;
    default: return 240;                                     // LZO
    }
}
// An execute on a stream of the CALLER's leaves an event behind it, so that alz_plan_results (which copies on the context's own,
// non-blocking stream) is ordered behind those kernels; executes on the context's stream are ordered by the stream itself.
static int plan_mark_done(alz_plan* p, hipStream_t s, bool foreign) {
    if (!foreign) { p->done_evt_set = false; return ALZ_OK; }
    if (!p->done_evt) HIP_TRY(hipEventCreateWithFlags(&p->done_evt, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(p->done_evt, s));
    p->done_evt_set = true;
    return ALZ_OK;
}
int alz_plan_execute(alz_ctx* c, alz_plan* p, const void* d_src_base, void* d_dst_base, void* hip_stream) {
    if (!c || !p) return fail(ALZ_E_INVALID, "alz_plan_execute: bad argument");
    HIP_TRY(hipSetDevice(c->device));                 // (a host thread may hold contexts of several devices)
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (p->big && !c->exact && c->variant == 0) {
        hipEvent_t* ev = p->big_borrowed ? &c->big_evt : &p->big_evt;
        bool* ev_set = p->big_borrowed ? &c->big_evt_set : &p->big_evt_set;
        if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        if (*ev_set) HIP_TRY(hipStreamWaitEvent(s, *ev, 0));           // (a no-op on the stream that recorded it; orders any other stream behind the last run)
        for (uint32_t i = 0; i < p->n; i++) {
            const int f = (int)p->big_streams[i].format;
            hipError_t e = alz_launch_big(f, s, d_src_base, d_dst_base, &p->big_streams[i], &p->lz, p->d_results + i, p->d_big, p->d_gate, c->d_big_accepted);
            if (e == hipSuccess) e = alz_launch_decode_gated(f, s, d_src_base, d_dst_base, p->d_streams, p->d_index + p->big_pos[i], 1, p->d_results, &p->lz, p->d_gate);
            if (e != hipSuccess) return fail(ALZ_E_HIP, "big-stream launch (format %d) failed: %s", f, hipGetErrorString(e));
            c->big_launches++;
        }
        HIP_TRY(hipEventRecord(*ev, s)); *ev_set = true;
        return plan_mark_done(p, s, s != c->stream);
    }
    int nfmt = 0;
    for (int f = 0; f < ALZ_FMT_COUNT; f++) nfmt += p->fmt_cnt[f] ? 1 : 0;
    // The work queues of this plan are in use by this execute: it starts behind the execute before it (the queue heads, flags and slots are the plan's, one set),
    // wherever that one was enqueued, and leaves the event for the next.  Plans without a queue only read their tables.
    const bool queued = p->d_tmo && !c->exact && (c->variant == 0 || c->variant == 3) && !p->no_chunks;
    const bool foreign = s != c->stream;
    if (queued) {
        // (executes on the context's own stream -- the usual case, and bench.py's -- are ordered by the stream and cost no event: a record per execute is a
        // barrier packet between the kernels of a 0.7 ms launch.  A stream of the caller's may be gone by the next call, so its event is recorded at once.)
        if (!p->q_evt) HIP_TRY(hipEventCreateWithFlags(&p->q_evt, hipEventDisableTiming));
        if (foreign && p->q_ctx_pending) { HIP_TRY(hipEventRecord(p->q_evt, c->stream)); p->q_evt_set = true; p->q_ctx_pending = false; }
        if (p->q_evt_set) { HIP_TRY(hipStreamWaitEvent(s, p->q_evt, 0)); if (!foreign) p->q_evt_set = false; }
        // this launch's epoch: what makes a hand-over flag count, and which of the two sets of queue heads is drawn from -- nothing is zeroed per launch.  When the
        // 30-bit counter comes round (a billion executes) everything is zeroed once, as at creation.
        if (p->epoch >= 0x3FFFFFFFu) {
            for (int f = 0; f < ALZ_FMT_COUNT; f++) if (p->chunk[f].n_items) HIP_TRY(hipMemsetAsync(p->chunk[f].d_ctl, 0, p->chunk[f].zero_bytes, s));
            p->epoch = 0;
        }
        p->epoch++;
    }
    // a format's launch: the work queue of chunks where the plan has one (and the context has not been switched to other kernels since), else one wavefront per stream
    auto launch_format = [&](int f, hipStream_t on) -> hipError_t {
        alz_plan::chunk_plan& cp = p->chunk[f];
        if (cp.n_items && queued) {
            hipError_t e = alz_launch_decode_chunked(f, on, d_src_base, d_dst_base, p->d_streams, cp.d_items, cp.n_items, &cp.bounds, p->d_results, &p->lz, cp.d_ctl, cp.d_flags, cp.d_slots, p->d_tmo + f, p->epoch);
            // ... and behind it the same streams with one wavefront per stream, gated by that word: workgroups that return at once (always, so far), or the whole repair in stream order
            if (e == hipSuccess) e = alz_launch_decode_gated(f, on, d_src_base, d_dst_base, p->d_streams, p->d_index + p->fmt_off[f], p->fmt_cnt[f], p->d_results, &p->lz, p->d_tmo + f);
            return e;
        }
        return alz_launch_decode(f, on, d_src_base, d_dst_base, p->d_streams, p->d_index + p->fmt_off[f], p->fmt_cnt[f], p->d_results, &p->lz, c->exact, p->n, c->variant);
    };
    if (nfmt <= 1) {
        for (int f = 0; f < ALZ_FMT_COUNT; f++) {
            if (!p->fmt_cnt[f]) continue;
            hipError_t e = launch_format(f, s);
            if (e != hipSuccess) return fail(ALZ_E_HIP, "kernel launch (format %d) failed: %s", f, hipGetErrorString(e));
        }
        if (queued) { if (foreign) { HIP_TRY(hipEventRecord(p->q_evt, s)); p->q_evt_set = true; } else p->q_ctx_pending = true; }
        return plan_mark_done(p, s, s != c->stream);
    }
    // mixed batch: one kernel per format, forked onto side streams so that they share the GPU (each format alone may
    // have far fewer streams than the device has wave slots), joined back into the caller's stream -- also when a launch
    // fails half way (the side streams that already started are joined, then the error is reported)
    // The format whose streams take longest ALONE goes first: a mixed launch is resident all at once and ends with its slowest
    // stream, and a stream's own time hardly depends on how many others of its format there are.
    // Four lanes: the caller's stream itself and three side streams.  Round 2 forked onto FOUR side streams; with the caller's
    // stream that made five, the HIP runtime maps streams onto four hardware queues, and rocprofv3 showed the fourth kernel of
    // the cfg4 shard waiting in the queue of the third until that had finished (3.09 ms for kernels of 2.2 / 1.8 / 1.8 / 1.3 ms).
    int order[ALZ_FMT_COUNT];
    for (int f = 0; f < ALZ_FMT_COUNT; f++) order[f] = f;
    std::stable_sort(order, order + ALZ_FMT_COUNT, [](int a, int b) { return format_latency((uint32_t)a) > format_latency((uint32_t)b); });
    HIP_TRY(hipEventRecord(c->fork, s));
    // Formats beyond the fourth queue up behind an earlier kernel: each goes to the lane with the least work queued so far (longest
    // first onto the least loaded lane; a kernel's share of the launch ~ its streams x the format's cost per byte) -- dealt round-robin,
    // the fifth format waited behind the slowest kernel of all while the faster lanes drained.
    int rc = ALZ_OK; bool used[4] = {false, false, false, false};
    uint64_t load[4] = {0, 0, 0, 0};
    for (int oi = 0; oi < ALZ_FMT_COUNT && rc == ALZ_OK; oi++) {
        const int f = order[oi];
        if (!p->fmt_cnt[f]) continue;
        int lane = 0;                                       // lane 0: the caller's stream; 1..3: side streams
        for (int l = 1; l < 4; l++) if (load[l] < load[lane]) lane = l;
        load[lane] += (uint64_t)p->fmt_cnt[f] * format_weight((uint32_t)f) + 1u;
        hipStream_t a = lane == 0 ? s : c->aux[lane - 1];
        if (lane != 0 && !used[lane]) {
            hipError_t w = hipStreamWaitEvent(a, c->fork, 0);
            if (w != hipSuccess) { rc = fail(ALZ_E_HIP, "hipStreamWaitEvent failed: %s", hipGetErrorString(w)); break; }
            used[lane] = true;
        }
        hipError_t e = launch_format(f, a);
        if (e != hipSuccess) rc = fail(ALZ_E_HIP, "kernel launch (format %d) failed: %s", f, hipGetErrorString(e));
    }
    for (int i = 1; i < 4; i++) if (used[i]) {
        hipError_t e = hipEventRecord(c->join[i], c->aux[i - 1]);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, c->join[i], 0);
        if (e != hipSuccess && rc == ALZ_OK) rc = fail(ALZ_E_HIP, "joining the side streams failed: %s", hipGetErrorString(e));
    }
    if (queued) {
        if (!foreign) p->q_ctx_pending = true;
        else { hipError_t e = hipEventRecord(p->q_evt, s); if (e == hipSuccess) p->q_evt_set = true; else if (rc == ALZ_OK) rc = fail(ALZ_E_HIP, "hipEventRecord failed: %s", hipGetErrorString(e)); }
    }
    if (rc == ALZ_OK) rc = plan_mark_done(p, s, s != c->stream);
    return rc;
}

int alz_plan_execute_timed(alz_ctx* c, alz_plan* p, const void* d_src_base, void* d_dst_base, int iters, float* mean_ms) {
    if (!c || !p || iters < 1 || !mean_ms) return fail(ALZ_E_INVALID, "alz_plan_execute_timed: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < iters; i++) { int rc = alz_plan_execute(c, p, d_src_base, d_dst_base, nullptr); if (rc) return rc; }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms = ms / (float)iters;
    c->last_kernel_ms = *mean_ms;
    return ALZ_OK;
}

int alz_plan_results(alz_ctx* c, alz_plan* p, alz_result* results) {
    if (!c || !p || (p->n && !results)) return fail(ALZ_E_INVALID, "alz_plan_results: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    if (p->done_evt_set) HIP_TRY(hipStreamWaitEvent(c->stream, p->done_evt, 0));    // (the last execute ran on a stream of the caller's)
    // the work queue's bounded spins: if one ever ran out (never seen), the gated launch behind that execute has already decoded the format again with one wavefront per
    // stream -- in stream order, so the results and every execute's bytes are whole -- and the word stays set: the plan leaves the queue for good
    uint32_t tmo[ALZ_FMT_COUNT] = {0};
    const bool look = p->d_tmo && !p->no_chunks;
    if (look) HIP_TRY(hipMemcpyAsync(tmo, p->d_tmo, sizeof(tmo), hipMemcpyDeviceToHost, c->stream));
    if (p->n) HIP_TRY(hipMemcpyAsync(results, p->d_results, p->n * sizeof(alz_result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (look) for (int f = 0; f < ALZ_FMT_COUNT; f++) if (tmo[f]) { p->no_chunks = true; c->chunk_repeats++; break; }
    return ALZ_OK;
}

// ---------------------------------------------------------------- host-buffer entry points
static int ensure_pinned(alz_ctx* c) {
    if (c->pin_cap) return ALZ_OK;
    for (int i = 0; i < 2; i++) {
        if (!c->pin[i]) HIP_TRY(hipHostMalloc(&c->pin[i], kPinBytes, hipHostMallocDefault));
        if (!c->pin_ev[i]) HIP_TRY(hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
    }
    if (!c->pool) c->pool = new (std::nothrow) copy_pool(copy_pool::default_threads());
    if (!c->pool) return fail(ALZ_E_NOMEM, "out of memory");
    c->pin_cap = kPinBytes;                                  // (set last: everything above exists from here on)
    return ALZ_OK;
}
// A pinned buffer is only touched by the host once the DMA recorded on it has completed -- also across calls: the flag lives in
// the context, so a second staging call that follows at once (or one that follows a call that returned early with an error)
// waits for the first call's DMA instead of overwriting its source.
static int pin_wait(alz_ctx* c, int k) {
    if (c->pin_busy[k]) { HIP_TRY(hipEventSynchronize(c->pin_ev[k])); c->pin_busy[k] = false; }
    return ALZ_OK;
}
static int pin_mark(alz_ctx* c, int k) {
    HIP_TRY(hipEventRecord(c->pin_ev[k], c->stream)); c->pin_busy[k] = true;
    return ALZ_OK;
}
// host (pageable) -> device through the two pinned buffers: the memcpy of piece k + 1 overlaps the DMA of piece k
static int staged_h2d(alz_ctx* c, void* d_dst, const uint8_t* h_src, size_t bytes) {
    if (!bytes) return ALZ_OK;
    if (bytes < (1u << 20) || ensure_pinned(c) != ALZ_OK) {
        HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, c->stream));
        return ALZ_OK;
    }
    size_t done = 0; int k = 0, rc;
    while (done < bytes) {
        const size_t n = bytes - done < c->pin_cap ? bytes - done : c->pin_cap;
        if ((rc = pin_wait(c, k))) return rc;
        c->copy((uint8_t*)c->pin[k], h_src + done, n);
        HIP_TRY(hipMemcpyAsync((uint8_t*)d_dst + done, c->pin[k], n, hipMemcpyHostToDevice, c->stream));
        if ((rc = pin_mark(c, k))) return rc;
        done += n; k ^= 1;
    }
    return ALZ_OK;
}
// device -> host (pageable), the same way: the DMA of piece k + 1 runs while piece k is copied out of its pinned buffer
static int staged_d2h(alz_ctx* c, uint8_t* h_dst, const void* d_src, size_t bytes) {
    if (!bytes) return ALZ_OK;
    if (bytes < (1u << 20) || ensure_pinned(c) != ALZ_OK) {
        HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return ALZ_OK;
    }
    size_t issued = 0, copied = 0; int k = 0, rc;
    size_t len[2] = {0, 0};
    {   const size_t n = bytes < c->pin_cap ? bytes : c->pin_cap;
        HIP_TRY(hipMemcpyAsync(c->pin[0], d_src, n, hipMemcpyDeviceToHost, c->stream));   // (stream order keeps it behind an earlier DMA out of pin[0])
        if ((rc = pin_mark(c, 0))) return rc;
        len[0] = n; issued = n; }
    while (copied < bytes) {
        if (issued < bytes) {
            const size_t n = bytes - issued < c->pin_cap ? bytes - issued : c->pin_cap;
            HIP_TRY(hipMemcpyAsync(c->pin[k ^ 1], (const uint8_t*)d_src + issued, n, hipMemcpyDeviceToHost, c->stream));
            if ((rc = pin_mark(c, k ^ 1))) return rc;
            len[k ^ 1] = n; issued += n;
        }
        if ((rc = pin_wait(c, k))) return rc;
        c->copy(h_dst + copied, (const uint8_t*)c->pin[k], len[k]);
        copied += len[k]; k ^= 1;
    }
    return ALZ_OK;
}

static int grow(alz_ctx* c, void** buf, size_t* cap, size_t need) {
    if (*cap >= need) return ALZ_OK;
    if (*buf) { HIP_TRY(hipFree(*buf)); *buf = nullptr; *cap = 0; }
    size_t want = need + need / 4 + 4096;
    HIP_TRY(hipMalloc(buf, want));
    *cap = want;
    return ALZ_OK;
}

// The part every host form shares: the library's own device buffers grown to the batch (64 bytes of read slack behind each), the source staged
static int stage_source(alz_ctx* c, const uint8_t* src, size_t src_bytes, bool has_dst, size_t dst_bytes) {
    int rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = grow(c, &c->d_src, &c->d_src_cap, src_bytes + 64))) return rc;
    if (has_dst && (rc = grow(c, &c->d_dst, &c->d_dst_cap, dst_bytes + 64))) return rc;
    return staged_h2d(c, c->d_src, src, src_bytes);
}

// Sparse outputs (compressed streams in worst-case-sized slots, batches with failed streams): one workgroup per stream packs
// the produced bytes into a dense device buffer, so that ONE copy crosses PCIe instead of one per stream.  `to` is congruent
// to `from` modulo 16, which keeps the 16-byte body of the copy aligned on both sides.
struct pack_item { uint64_t from, to; uint32_t len, pad; };
__global__ void __launch_bounds__(256) alz_pack_outputs_kernel(const uint8_t* __restrict__ base, uint8_t* __restrict__ pack, const pack_item* __restrict__ items) {
    const pack_item it = items[blockIdx.x];
    const uint8_t* s = base + it.from;
    uint8_t* d = pack + it.to;
    uint32_t head = (16u - (uint32_t)(it.from & 15)) & 15u;
    if (head > it.len) head = it.len;
    for (uint32_t k = threadIdx.x; k < head; k += blockDim.x) d[k] = s[k];
    const uint32_t body = (it.len - head) >> 4;
    const uint4* s4 = (const uint4*)(s + head);
    uint4* d4 = (uint4*)(d + head);
    for (uint32_t k = threadIdx.x; k < body; k += blockDim.x) d4[k] = s4[k];
    for (uint32_t k = head + (body << 4) + threadIdx.x; k < it.len; k += blockDim.x) d[k] = s[k];
}

// one produced range: `len` bytes at device offset `dev` (relative to ctx->d_dst) that belong at `host`
struct out_seg { uint64_t dev; uint8_t* host; uint32_t len; };

// false = could not pack (no device memory for the dense copy): the caller falls back to one copy per stream
// Segments sorted by `dev` (offsets relative to d_base), pinned buffers present: windows of the device range go through the two
// pinned buffers -- the DMA of window w + 1 overlaps the copy-out of window w, which the context's copy threads spread.  Only
// the segments' own bytes are written on the host side.
static int download_windows(alz_ctx* c, const void* d_base, const std::vector<out_seg>& segs) {
    uint64_t lo = segs.front().dev, hi = 0;
    for (const out_seg& g : segs) if (g.dev + g.len > hi) hi = g.dev + g.len;
    const uint64_t W = c->pin_cap;
    const uint64_t nwin = (hi - lo + W - 1) / W;
    size_t first = 0;                                        // first segment that may still overlap the current window
    auto issue = [&](uint64_t w, int k) -> hipError_t {
        const uint64_t a = lo + w * W, n = hi - a < W ? hi - a : W;
        hipError_t e = hipMemcpyAsync(c->pin[k], (const uint8_t*)d_base + a, n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipEventRecord(c->pin_ev[k], c->stream);
        if (e == hipSuccess) c->pin_busy[k] = true;
        return e;
    };
    HIP_TRY(issue(0, 0));
    for (uint64_t w = 0; w < nwin; w++) {
        const int k = (int)(w & 1);
        if (w + 1 < nwin) HIP_TRY(issue(w + 1, k ^ 1));
        { const int rcw = pin_wait(c, k); if (rcw) return rcw; }
        const uint64_t a = lo + w * W, b = a + W;
        while (first < segs.size() && segs[first].dev + segs[first].len <= a) first++;
        c->jobs.clear();
        for (size_t i = first; i < segs.size() && segs[i].dev < b; i++) {
            const uint64_t s0 = segs[i].dev > a ? segs[i].dev : a, s1 = segs[i].dev + segs[i].len < b ? segs[i].dev + segs[i].len : b;
            if (s1 > s0) add_copy(c->jobs, segs[i].host + (s0 - segs[i].dev), (const uint8_t*)c->pin[k] + (s0 - a), s1 - s0);
        }
        c->pool->run(c->jobs);
    }
    return ALZ_OK;
}

// false = could not pack (no device memory for the dense copy, no pinned memory): the caller falls back to one copy per stream
static bool download_packed(alz_ctx* c, const std::vector<out_seg>& segs) {
    if (ensure_pinned(c) != ALZ_OK) { (void)hipGetLastError(); return false; }
    std::vector<pack_item> items;
    std::vector<out_seg> packed;                             // the same segments at their offsets in the dense copy
    items.reserve(segs.size()); packed.reserve(segs.size());
    uint64_t cur = 0;
    for (const out_seg& g : segs) {
        const uint64_t to = cur + (g.dev & 15);
        items.push_back(pack_item{g.dev, to, g.len, 0});
        packed.push_back(out_seg{to, g.host, g.len});
        cur = (to + g.len + 15) & ~15ull;
    }
    // (scratch of the context, grown on demand: no hipMalloc / hipFree per call)
    if (grow(c, &c->d_items, &c->d_items_cap, items.size() * sizeof(pack_item)) != ALZ_OK) { (void)hipGetLastError(); return false; }
    if (grow(c, &c->d_pack, &c->d_pack_cap, cur + 16) != ALZ_OK) { (void)hipGetLastError(); return false; }
    hipError_t e = hipMemcpyAsync(c->d_items, items.data(), items.size() * sizeof(pack_item), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        alz_pack_outputs_kernel<<<dim3((uint32_t)items.size()), dim3(256), 0, c->stream>>>((const uint8_t*)c->d_dst, (uint8_t*)c->d_pack, (const pack_item*)c->d_items);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    // (items is read by the asynchronous upload above: the first window's event wait below orders the two)
    if (download_windows(c, c->d_pack, packed) != ALZ_OK) { (void)hipGetLastError(); return false; }
    return true;
}

// Download the produced ranges: through the pinned staging buffers window by window when they are reasonably dense (the
// caller's bytes between streams are never touched), else packed on the device first.
static int download_segs(alz_ctx* c, std::vector<out_seg>& segs) {
    if (segs.empty()) return ALZ_OK;
    std::sort(segs.begin(), segs.end(), [](const out_seg& a, const out_seg& b) { return a.dev < b.dev; });
    uint64_t lo = segs.front().dev, hi = 0, sum = 0;
    for (const out_seg& g : segs) { if (g.dev + g.len > hi) hi = g.dev + g.len; sum += g.len; }
    if (hi - lo > 2 * sum + (64ull << 20)) {
        if (segs.size() >= 16 && download_packed(c, segs)) return ALZ_OK;
        for (const out_seg& g : segs) HIP_TRY(hipMemcpyAsync(g.host, (const uint8_t*)c->d_dst + g.dev, g.len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return ALZ_OK;
    }
    if (ensure_pinned(c) != ALZ_OK) {                        // no pinned memory: one bounce buffer
        std::vector<uint8_t> bounce(hi - lo);
        HIP_TRY(hipMemcpyAsync(bounce.data(), (const uint8_t*)c->d_dst + lo, hi - lo, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (const out_seg& g : segs) memcpy(g.host, bounce.data() + (g.dev - lo), g.len);
        return ALZ_OK;
    }
    return download_windows(c, c->d_dst, segs);
}

// crilayla_top: the batch is one of alz_bitlz_kind, and a CRILAYLA stream's bytes lie at the TOP of its span
static int download_outputs(alz_ctx* c, uint32_t n, const alz_stream* streams, const alz_result* results, uint8_t* dst_base, bool only_ok, bool crilayla_top = false) {
    std::vector<out_seg> segs;
    segs.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        if (!results[i].dst_len || (only_ok && results[i].status != ALZ_ST_OK)) continue;
        const uint64_t at = streams[i].dst_off + (crilayla_top && streams[i].format == ALZ_BITLZ_CRILAYLA ? streams[i].dst_cap - results[i].dst_len : 0u);
        segs.push_back(out_seg{at, dst_base + at, results[i].dst_len});
    }
    return download_segs(c, segs);
}

int alz_decode_batch(alz_ctx* c, const alz_lz_properties* props, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                     const alz_stream* streams, uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    if (!c || (n && (!streams || !results))) return fail(ALZ_E_INVALID, "alz_decode_batch: bad argument");
    int rc;   // (the ranges of every stream first; the plan refuses an unknown format behind them)
    if ((rc = validate_streams("", 0, n, streams, &src_bytes, &dst_bytes, [](uint32_t i, const alz_stream& s) -> int {   // (as alz_decode_batch_multi: the history lies in front of the block's output)
            return lz4_history_outside(s) ? fail(ALZ_E_INVALID, "stream %u: LZ4 history (aux0) reaches in front of the destination buffer", i) : ALZ_OK;
        }))) return rc;
    if ((rc = stage_source(c, src_base, src_bytes, true, dst_bytes))) return rc;
    for (uint32_t i = 0; i < n; i++)   // LZ4 blocks that continue a frame's window: their history has to be in HBM too
        if (streams[i].format == ALZ_FMT_LZ4_BLOCK && streams[i].aux0 && streams[i].aux0 <= streams[i].dst_off)
            HIP_TRY(hipMemcpyAsync((uint8_t*)c->d_dst + streams[i].dst_off - streams[i].aux0, dst_base + streams[i].dst_off - streams[i].aux0,
                                   streams[i].aux0, hipMemcpyHostToDevice, c->stream));
    alz_plan* p = nullptr;
    if ((rc = plan_create(c, props, n, streams, &p, true))) return rc;
    rc = alz_plan_execute(c, p, c->d_src, c->d_dst, nullptr);
    // ONE stream that states its size (what a format class's Decompress(Stream, Stream) hands over): the output travels with the result --
    // one wait instead of two (0.254 against 0.261 ms per call, A/B in one run) -- and what the stream really produced is copied out of the staging buffer
    const uint32_t spec = (n == 1 && streams[0].decom_len) ? (streams[0].decom_len < streams[0].dst_cap ? streams[0].decom_len : streams[0].dst_cap) : 0u;
    if (!rc && spec && spec <= kPinBytes && ensure_pinned(c) == ALZ_OK) {
        if ((rc = pin_wait(c, 0)) == ALZ_OK) {
            hipError_t e = hipMemcpyAsync(results, p->d_results, sizeof(alz_result), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c->pin[0], (const uint8_t*)c->d_dst + streams[0].dst_off, spec, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(ALZ_E_HIP, "download failed: %s", hipGetErrorString(e));
        }
        if (!rc) {
            if (results[0].dst_len <= spec) { if (results[0].dst_len) memcpy(dst_base + streams[0].dst_off, c->pin[0], results[0].dst_len); }
            else rc = download_outputs(c, n, streams, results, dst_base, false);         // (an overshoot of the declared size: E4)
        }
    } else {
        if (!rc) rc = alz_plan_results(c, p, results);
        if (!rc) rc = download_outputs(c, n, streams, results, dst_base, false);   // copy back only what each stream produced
    }
    if (rc) (void)hipStreamSynchronize(c->stream);           // (an error path: the plan's pageable upload sources may still be queued)
    alz_plan_destroy(c, p);
    return rc;
}

int alz_decode(alz_ctx* c, uint32_t format, const alz_lz_properties* props, const uint8_t* src, uint32_t src_len, uint32_t decom_len,
               uint32_t aux0, uint32_t aux1, uint8_t* dst, uint32_t dst_cap, alz_result* result) {
    if (!result) return fail(ALZ_E_INVALID, "alz_decode: result is NULL");
    alz_stream s; memset(&s, 0, sizeof(s));
    s.src_len = src_len; s.dst_cap = dst_cap; s.decom_len = decom_len; s.aux0 = aux0; s.aux1 = aux1; s.format = format;
    return alz_decode_batch(c, props, 1, src, src_len, &s, dst, dst_cap, result);
}

// ---------------------------------------------------------------- the batch core of the entry-point families that have no plan object
// measure (alz_measure.hip), RLE30 / HUF20 (alz_rlh.hip), aPLib (alz_aplib.hip), CRILAYLA / ALLZ (alz_bitlz.hip) and DEFLATE (alz_inflate.hip).  One call is one batch,
// grouped per kind like a plan (one launch per kind present, longest streams first inside a launch), on the context's stream; the three
// tables live in the context's plan scratch and the results come back to the host.  A family supplies its name, the number of kinds its
// `format` field selects among (1: the field is ignored), which bytes its host form downloads, the refusals only it has, and its launch.
extern "C++" {   // (templates)
enum batch_download {
    DL_NO_DST,            // a measure family: no destination, dst_off is not looked at and dst_cap only bounds the count
    DL_PRODUCED,          // [dst_off, dst_off + dst_len) of every stream, whatever its status (as alz_decode_batch)
    DL_ONLY_OK,           // ... of the streams that are ALZ_ST_OK (an encoder: as alz_encode_batch)
    DL_CRILAYLA_TOP       // DL_PRODUCED, but a CRILAYLA stream's bytes END at dst_off + dst_cap (it is written from the top down)
};
// the arguments every one of these entry points takes; src / dst are device pointers in a device form (dst NULL where there is none)
struct batch_args { uint32_t n; const uint8_t* src; size_t src_bytes; const alz_stream* streams; uint8_t* dst; size_t dst_bytes; alz_result* results; };
static int no_refusals() { return ALZ_OK; }

// n > 0 validated streams: group, sort, upload the tables, one launch(kind, d_streams, d_index of the kind, count, d_results) -> hipError_t per
// kind present between the two events, results to the host, wait.
template <class Launch>
static int grouped_core(alz_ctx* c, const char* what, uint32_t kinds, uint32_t n, const alz_stream* streams, alz_result* results, Launch launch) {
    uint32_t cnt[kMaxKinds], off[kMaxKinds]; std::vector<uint32_t> index;
    c->last_kernel_ms = 0.f;
    HIP_TRY(hipSetDevice(c->device));
    group_streams(n, kinds, [&](uint32_t i) { return kinds > 1 ? streams[i].format : 0u; },
                  [&](uint32_t i) { return streams[i].src_len; }, index, off, cnt);     // a stream's cost is its tokens: the compressed bytes
    plan_tables t;
    if (int rc = carve_plan_scratch(c, n, &t)) return rc;
    return launch_bracket(c, what,
        [&] {   // (the uploads read the caller's table and `index`: the bracket waits for them)
            hipError_t e = hipMemcpyAsync(t.streams, streams, (size_t)n * sizeof(alz_stream), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(t.index, index.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemsetAsync(t.results, 0xFF, (size_t)n * sizeof(alz_result), c->stream);
            return e;
        },
        [&] { hipError_t e = hipSuccess; for (uint32_t f = 0; f < kinds && e == hipSuccess; f++) if (cnt[f]) e = launch(f, t.streams, t.index + off[f], cnt[f], t.results); return e; },
        [&] { return hipMemcpyAsync(results, t.results, (size_t)n * sizeof(alz_result), hipMemcpyDeviceToHost, c->stream); });
}

// One entry point, host or device form: the argument check, the empty batch, validation (once, before anything is allocated or copied: a
// refused call pays for no upload), the host form's staging of the source, the core, the host form's download.
// refuse() -> int: the family's own refusals; launch(kind, d_src, d_dst, d_streams, d_index, count, d_results) -> hipError_t.
template <class Refuse, class Launch>
static int batch_call(alz_ctx* c, const char* what, uint32_t kinds, batch_download rule, bool device, const batch_args& a, Refuse refuse, Launch launch) {
    const bool has_dst = rule != DL_NO_DST;
    const bool missing = device ? a.n && (!a.streams || !a.results || !a.src || (has_dst && !a.dst))
                                : (a.n && (!a.streams || !a.results)) || (a.src_bytes && !a.src) || (has_dst && a.dst_bytes && !a.dst);
    if (!c || missing) return fail(ALZ_E_INVALID, "%s: bad argument", what);
    if (a.n == 0) { c->last_kernel_ms = 0.f; return ALZ_OK; }
    int rc;
    if ((rc = validate_streams(what, kinds, a.n, a.streams, &a.src_bytes, has_dst ? &a.dst_bytes : nullptr, no_refusal))) return rc;
    if ((rc = refuse())) return rc;
    const uint8_t* d_src = a.src; uint8_t* d_dst = a.dst;
    if (!device) {
        if ((rc = stage_source(c, a.src, a.src_bytes, has_dst, a.dst_bytes))) return rc;
        d_src = (const uint8_t*)c->d_src;
        d_dst = has_dst ? (uint8_t*)c->d_dst : nullptr;
    }
    rc = grouped_core(c, what, kinds, a.n, a.streams, a.results, [&](uint32_t kind, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
        return launch(kind, d_src, d_dst, d_streams, d_index, count, d_results);
    });
    if (rc || device || !has_dst) return rc;
    return download_outputs(c, a.n, a.streams, a.results, a.dst, rule == DL_ONLY_OK, rule == DL_CRILAYLA_TOP);
}

// The core of the families over byte ranges (the checksums and XXH32, below), host or device form: the argument check, the empty batch, validation, the
// host form's staging, the tables -- ranges | the family's own | one word per range -- carved out of the plan scratch, one timed launch, the words
// back to the host.  check(i, range) -> int: the family's refusal per range, behind the range's own; own_bytes() -> size_t: the bytes of its tables
// (asked once the ranges are valid); upload(d_own) and launch(d_src, d_ranges, d_own, d_out) -> hipError_t.
struct range_args { uint32_t n; const uint8_t* src; size_t src_bytes; const alz_stream* ranges; uint32_t* out; };
template <class Check, class OwnBytes, class Upload, class Launch>
static int range_call(alz_ctx* c, const char* what, bool device, const range_args& a, Check check, OwnBytes own_bytes, Upload upload, Launch launch) {
    const bool missing = device ? a.n && (!a.ranges || !a.out || !a.src) : (a.n && (!a.ranges || !a.out)) || (a.src_bytes && !a.src);
    if (!c || missing) return fail(ALZ_E_INVALID, "%s: bad argument", what);
    if (a.n == 0) { c->last_kernel_ms = 0.f; return ALZ_OK; }
    int rc;
    if ((rc = validate_streams(what, 0, a.n, a.ranges, &a.src_bytes, nullptr, check, true))) return rc;
    c->last_kernel_ms = 0.f;
    if (device) HIP_TRY(hipSetDevice(c->device));
    else if ((rc = stage_source(c, a.src, a.src_bytes, false, 0))) return rc;
    const uint8_t* d_src = device ? a.src : (const uint8_t*)c->d_src;
    const size_t r = ((size_t)a.n * sizeof(alz_stream) + 255) & ~(size_t)255, own = own_bytes();
    if ((rc = grow(c, &c->d_plan, &c->d_plan_cap, r + own + (size_t)a.n * sizeof(uint32_t)))) return rc;
    alz_stream* d_ranges = (alz_stream*)c->d_plan;
    uint8_t* d_own = (uint8_t*)c->d_plan + r; uint32_t* d_out = (uint32_t*)(d_own + own);
    return launch_bracket(c, what,   // (the uploads read the caller's table and the family's: the bracket waits for them)
        [&] { const hipError_t e = hipMemcpyAsync(d_ranges, a.ranges, (size_t)a.n * sizeof(alz_stream), hipMemcpyHostToDevice, c->stream); return e == hipSuccess ? upload(d_own) : e; },
        [&] { return launch(d_src, d_ranges, d_own, d_out); },
        [&] { return hipMemcpyAsync(a.out, d_out, (size_t)a.n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream); });
}
}   // extern "C++"

// ---------------------------------------------------------------- measure: decoded sizes without decoding (alz_measure.hip); kinds: alz_format
static int measure_batch(alz_ctx* c, bool device, const alz_lz_properties* props, const batch_args& a) {
    const alz_lz_properties lz = effective_lz(props);
    return batch_call(c, "alz_measure_batch", ALZ_FMT_COUNT, DL_NO_DST, device, a,
        [&]() -> int {
            for (uint32_t i = 0; i < a.n && !lzss_on_gpu(lz); i++)
                if (a.streams[i].format == ALZ_FMT_LZSS) return fail(ALZ_E_UNSUPPORTED, "LZSS geometry outside the GPU path (window_bits 8..16, length_bits 1..8)");
            return ALZ_OK;
        },
        [&](uint32_t f, const uint8_t* d_src, uint8_t*, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return alz_launch_measure((int)f, c->stream, d_src, d_streams, d_index, count, d_results, &lz, c->exact);
        });
}
int alz_measure_batch(alz_ctx* c, const alz_lz_properties* props, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                      const alz_stream* streams, alz_result* results) {
    return measure_batch(c, false, props, {n, src_base, src_bytes, streams, nullptr, 0, results});
}
int alz_measure_batch_device(alz_ctx* c, const alz_lz_properties* props, uint32_t n, const uint8_t* d_src_base, size_t src_bytes,
                             const alz_stream* streams, alz_result* results) {
    return measure_batch(c, true, props, {n, d_src_base, src_bytes, streams, nullptr, 0, results});
}

// ---------------------------------------------------------------- RLE30 / HUF20: the non-LZ bodies of the GBA / DS family (alz_rlh.hip); kinds: alz_rlh_format
static int rlh_batch(alz_ctx* c, bool device, bool encode, const batch_args& a) {
    const char* what = encode ? "alz_rlh_encode_batch" : "alz_rlh_decode_batch";
    return batch_call(c, what, ALZ_RLH_COUNT, encode ? DL_ONLY_OK : DL_PRODUCED, device, a,
        [&]() -> int {
            for (uint32_t i = 0; i < a.n; i++) {
                if (a.streams[i].format == ALZ_RLH_RLE30) continue;
                // HuffmanTree.CreateTree sorts equal frequencies with the unstable List.Sort(): the managed bytes are not a function of the input
                if (encode) return fail(ALZ_E_UNSUPPORTED, "%s: stream %u: HUF20 has no encoder (the managed output is not a function of its input)", what, i);
                if (a.streams[i].decom_len >= 0x10000000u)   // symbolsToDecompress = destination.Length * 8 / bitDepth overflows the managed int  HUF20.cs:117
                    return fail(ALZ_E_UNSUPPORTED, "%s: stream %u: HUF20 decom_len >= 0x10000000", what, i);
            }
            return ALZ_OK;
        },
        [&](uint32_t f, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return encode ? alz_launch_rlh_encode((int)f, c->stream, d_src, d_dst, d_streams, d_index, count, d_results, c->exact)
                          : alz_launch_rlh_decode((int)f, c->stream, d_src, d_dst, d_streams, d_index, count, d_results, c->exact);
        });
}
int alz_rlh_decode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                         uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return rlh_batch(c, false, false, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_rlh_encode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                         uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return rlh_batch(c, false, true, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_rlh_decode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return rlh_batch(c, true, false, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}
int alz_rlh_encode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return rlh_batch(c, true, true, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}

// ---------------------------------------------------------------- RLHudson: RLE30's sibling of the HudsonSoft assembly (alz_rlh.hip)
// Decode and encode.  One kind: `format`, aux0 and aux1 of a stream are ignored.
size_t alz_rlhudson_encode_bound(size_t src_len) { return 2 * src_len; }   // a token never has more bytes than twice what it covers (a run of 3: 2, one literal: 2)

static int rlhudson_batch(alz_ctx* c, bool device, bool encode, const batch_args& a) {
    return batch_call(c, encode ? "alz_rlhudson_encode_batch" : "alz_rlhudson_decode_batch", 1, encode ? DL_ONLY_OK : DL_PRODUCED, device, a, no_refusals,
        [&](uint32_t, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return encode ? alz_launch_rlhudson_encode(c->stream, d_src, d_dst, d_streams, d_index, count, d_results)
                          : alz_launch_rlhudson_decode(c->stream, d_src, d_dst, d_streams, d_index, count, d_results, c->exact);
        });
}
int alz_rlhudson_decode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                              uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return rlhudson_batch(c, false, false, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_rlhudson_encode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                              uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return rlhudson_batch(c, false, true, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_rlhudson_decode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                     uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return rlhudson_batch(c, true, false, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}
int alz_rlhudson_encode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                     uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return rlhudson_batch(c, true, true, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}

// ---------------------------------------------------------------- aPLib: the last LzWindows user (alz_aplib.hip)
// Decode and measure.  One kind: `format`, decom_len, aux0 and aux1 of a stream are ignored.
static int aplib_batch(alz_ctx* c, bool device, bool measure, const batch_args& a) {
    return batch_call(c, measure ? "alz_aplib_measure_batch" : "alz_aplib_decode_batch", 1, measure ? DL_NO_DST : DL_PRODUCED, device, a, no_refusals,
        [&](uint32_t, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return measure ? alz_launch_aplib_measure(c->stream, d_src, d_streams, d_index, count, d_results)
                           : alz_launch_aplib_decode(c->stream, d_src, d_dst, d_streams, d_index, count, d_results,
                                                     c->exact ? ALZ_APLIB_EXACT : (c->variant != 0 ? ALZ_APLIB_PRODUCTION : ALZ_APLIB_DEFAULT));
        });
}
int alz_aplib_decode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return aplib_batch(c, false, false, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_aplib_decode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                  uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return aplib_batch(c, true, false, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}
int alz_aplib_measure_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams, alz_result* results) {
    return aplib_batch(c, false, true, {n, src_base, src_bytes, streams, nullptr, 0, results});
}
int alz_aplib_measure_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams, alz_result* results) {
    return aplib_batch(c, true, true, {n, d_src_base, src_bytes, streams, nullptr, 0, results});
}

// ---------------------------------------------------------------- CRILAYLA / ALLZ: the bit-stream LZ bodies of the .Extended assembly (alz_bitlz.hip)
// Decode only; kinds: alz_bitlz_kind.  Each kind has one kernel, so all three context modes run it.
static int bitlz_batch(alz_ctx* c, bool device, const batch_args& a) {
    return batch_call(c, "alz_bitlz_decode_batch", ALZ_BITLZ_COUNT, DL_CRILAYLA_TOP, device, a, no_refusals,
        [&](uint32_t kind, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return alz_launch_bitlz_decode((int)kind, c->stream, d_src, d_dst, d_streams, d_index, count, d_results);
        });
}
int alz_bitlz_decode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return bitlz_batch(c, false, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_bitlz_decode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                  uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return bitlz_batch(c, true, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}

// ---------------------------------------------------------------- DEFLATE: zlib's inflate over raw streams (alz_inflate.hip)
// Decode and measure.  One kind: `format`, decom_len, aux0 and aux1 of a stream are ignored.  One kernel each, so all three context modes run it.
static int inflate_batch(alz_ctx* c, bool device, bool measure, const batch_args& a) {
    return batch_call(c, measure ? "alz_inflate_measure_batch" : "alz_inflate_decode_batch", 1, measure ? DL_NO_DST : DL_PRODUCED, device, a, no_refusals,
        [&](uint32_t, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t* d_index, uint32_t count, alz_result* d_results) {
            return measure ? alz_launch_inflate_measure(c->stream, d_src, d_streams, d_index, count, d_results)
                           : alz_launch_inflate_decode(c->stream, d_src, d_dst, d_streams, d_index, count, d_results);
        });
}
int alz_inflate_decode_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                             uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return inflate_batch(c, false, false, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_inflate_decode_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                    uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return inflate_batch(c, true, false, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}
int alz_inflate_measure_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams, alz_result* results) {
    return inflate_batch(c, false, true, {n, src_base, src_bytes, streams, nullptr, 0, results});
}
int alz_inflate_measure_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams, alz_result* results) {
    return inflate_batch(c, true, true, {n, d_src_base, src_bytes, streams, nullptr, 0, results});
}

// ---------------------------------------------------------------- DEFLATE, the other direction (alz_inflate.hip, alz_inflate.h): alz_deflate_*
// One kind; every context mode runs the same kernels.  The host cuts the streams into blocks; the block table, the plans and the tokens
// (one word per input byte) live in the context's encoder scratch.
size_t alz_deflate_bound(size_t src_len) {
    const size_t blocks = src_len ? (src_len + ALZ_DEFLATE_BLOCK - 1) / ALZ_DEFLATE_BLOCK : 1;
    return src_len + 5 * blocks;                             // every block is at most its stored form
}
int alz_deflate_block_bytes(void) { return (int)ALZ_DEFLATE_BLOCK; }

static int deflate_batch(alz_ctx* c, bool device, int level, uint32_t flags, const batch_args& a) {
    const char* what = device ? "alz_deflate_encode_batch_device" : "alz_deflate_encode_batch";
    if (level < 0 || level > 9) return fail(ALZ_E_INVALID, "%s: level %d is not 0..9", what, level);
    if (flags & ~ALZ_DEFLATE_FIXED) return fail(ALZ_E_INVALID, "%s: unknown flags 0x%x", what, flags);
    std::vector<alz_deflate_blk> blocks;                     // (outlive the launches: grouped_core waits for the stream)
    std::vector<uint32_t> first;
    return batch_call(c, what, 1, DL_ONLY_OK, device, a,
        [&]() -> int {
            for (uint32_t i = 0; i < a.n; i++)
                if (a.streams[i].src_len >= 0x7FFFFF00u) return fail(ALZ_E_UNSUPPORTED, "%s: stream %u: 0x7FFFFF00 bytes and more", what, i);
            return ALZ_OK;
        },
        [&](uint32_t, const uint8_t* d_src, uint8_t* d_dst, const alz_stream* d_streams, const uint32_t*, uint32_t, alz_result* d_results) -> hipError_t {
            uint64_t tok = 0;
            first.resize((size_t)a.n + 1);
            for (uint32_t i = 0; i < a.n; i++) {
                first[i] = (uint32_t)blocks.size();
                const uint32_t len = a.streams[i].src_len, nb = len ? (len + ALZ_DEFLATE_BLOCK - 1) / ALZ_DEFLATE_BLOCK : 1u;
                if (blocks.size() + nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
                for (uint32_t k = 0; k < nb; k++) blocks.push_back(alz_deflate_blk{i, k, tok + (uint64_t)k * ALZ_DEFLATE_BLOCK});
                tok += len;
            }
            first[a.n] = (uint32_t)blocks.size();
            const size_t nblk = blocks.size();
            const size_t o_first = (nblk * sizeof(alz_deflate_blk) + 15) & ~(size_t)15, o_plans = (o_first + first.size() * 4 + 15) & ~(size_t)15,
                         o_tok = (o_plans + nblk * sizeof(alz_deflate_plan) + 15) & ~(size_t)15;
            if (grow(c, &c->enc_buf[alz_ctx::ENC_DEFLATE], &c->enc_cap[alz_ctx::ENC_DEFLATE], o_tok + (size_t)tok * 4 + 16) != ALZ_OK) return hipErrorOutOfMemory;
            uint8_t* base = (uint8_t*)c->enc_buf[alz_ctx::ENC_DEFLATE];
            hipError_t e = hipMemcpyAsync(base, blocks.data(), nblk * sizeof(alz_deflate_blk), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(base + o_first, first.data(), first.size() * 4, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) return e;
            return alz_launch_deflate_encode(c->stream, d_src, d_dst, d_streams, a.n, (const alz_deflate_blk*)base, (uint32_t)nblk, (const uint32_t*)(base + o_first),
                                             (uint32_t*)(base + o_tok), (alz_deflate_plan*)(base + o_plans), level, flags, d_results);
        });
}
int alz_deflate_encode_batch(alz_ctx* c, int level, uint32_t flags, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                             uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return deflate_batch(c, false, level, flags, {n, src_base, src_bytes, streams, dst_base, dst_bytes, results});
}
int alz_deflate_encode_batch_device(alz_ctx* c, int level, uint32_t flags, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                    uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return deflate_batch(c, true, level, flags, {n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results});
}

// ---------------------------------------------------------------- checksums: Adler-32 and CRC-32 of byte ranges (alz_checksum.hip); kinds: alz_checksum_kind
// A range is src_off / src_len of its alz_stream, nothing else.  The tables (ranges, chunk prefix, chunk sums, results) live in the context's plan
// scratch; the device writes nothing but them.
static uint32_t g_checksum_chunk = ALZ_CHECKSUM_CHUNK;
int alz_debug_checksum_chunk(uint32_t bytes) {   // bytes of a range one wavefront sums, for every context: 0 asks, a multiple of 1024 up to 1 MiB sets; returns the value in force
    if (bytes && bytes % 1024u == 0 && bytes <= ALZ_CHECKSUM_CHUNK_MAX) g_checksum_chunk = bytes;
    return (int)g_checksum_chunk;
}
// kind: an alz_checksum_kind, or ALZ_CK_CRC32C (alz_checksum.h) from the alz_crc32c_* entry points below.  Its own tables: first[] (n + 1 words: where
// a range's chunks start) | one partial sum per chunk
static int checksum_batch(alz_ctx* c, bool device, uint32_t kind, const range_args& a) {
    const bool crc32c = kind == ALZ_CK_CRC32C;
    const char* what = crc32c ? (device ? "alz_crc32c_batch_device" : "alz_crc32c_batch") : (device ? "alz_checksum_batch_device" : "alz_checksum_batch");
    const uint32_t chunk = g_checksum_chunk;
    std::vector<uint32_t> first; uint64_t total = 0;
    const size_t b = (((size_t)a.n + 1) * sizeof(uint32_t) + 255) & ~(size_t)255;
    return range_call(c, what, device, a,
        [&](uint32_t i, const alz_stream& r) -> int {
            if (i == 0) first.resize((size_t)a.n + 1);          // (here, not above: the arguments have been checked)
            first[i] = (uint32_t)total; total += ((uint64_t)r.src_len + chunk - 1) / chunk;
            return total > 0x7FFFFFFFull ? fail(ALZ_E_UNSUPPORTED, "%s: more than 2^31 chunks of %u bytes", what, chunk) : ALZ_OK;
        },
        [&] { first[a.n] = (uint32_t)total; return b + (((size_t)total * sizeof(uint32_t) + 255) & ~(size_t)255); },
        [&](uint8_t* d_own) { return hipMemcpyAsync(d_own, first.data(), ((size_t)a.n + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream); },
        [&](const uint8_t* d_src, const alz_stream* d_ranges, uint8_t* d_own, uint32_t* d_out) {
            return alz_launch_checksum(kind, c->stream, d_src, d_ranges, a.n, (const uint32_t*)d_own, (uint32_t)total, chunk, (uint32_t*)(d_own + b), d_out);
        });
}
// (the public kinds end at CRC-32: the launcher's third kind has entry points of its own, and 2 stays an unknown kind here)
int alz_checksum_batch(alz_ctx* c, uint32_t kind, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    if (kind > ALZ_CK_CRC32) return fail(ALZ_E_INVALID, "alz_checksum_batch: unknown kind %u", kind);
    return checksum_batch(c, false, kind, {n, src_base, src_bytes, ranges, out});
}
int alz_checksum_batch_device(alz_ctx* c, uint32_t kind, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    if (kind > ALZ_CK_CRC32) return fail(ALZ_E_INVALID, "alz_checksum_batch_device: unknown kind %u", kind);
    return checksum_batch(c, true, kind, {n, d_src_base, src_bytes, ranges, out});
}
// the checksum of A || B from those of A and of B: pure host code, the arithmetic of the fold kernel (alz_checksum.h).  An unknown kind gives 0.
uint32_t alz_checksum_combine(uint32_t kind, uint32_t a, uint32_t b, uint64_t len_b) {
    if (kind > ALZ_CK_CRC32) return 0;
    return alz_checksum_join(kind, a, b, len_b, kind == ALZ_CK_CRC32 ? alz_crc_xpow_bytes(len_b) : 0u);
}

// CRC-32C (Castagnoli; the checksum of the framed Snappy container, before its mask): the same batch over the other polynomial
int alz_crc32c_batch(alz_ctx* c, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    return checksum_batch(c, false, ALZ_CK_CRC32C, {n, src_base, src_bytes, ranges, out});
}
int alz_crc32c_batch_device(alz_ctx* c, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    return checksum_batch(c, true, ALZ_CK_CRC32C, {n, d_src_base, src_bytes, ranges, out});
}
uint32_t alz_crc32c_combine(uint32_t a, uint32_t b, uint64_t len_b) {
    return alz_checksum_join(ALZ_CK_CRC32C, a, b, len_b, alz_crc_xpow_bytes<ALZ_CRC32C_POLY>(len_b));
}

// ---------------------------------------------------------------- XXH32 of byte ranges (alz_xxh32.hip): the argument rules of the checksum family
// One launch, four lanes per range.  The tables (ranges, results) live in the context's plan scratch; the device writes nothing but them.
static int xxh32_batch(alz_ctx* c, bool device, uint32_t seed, const range_args& a) {
    return range_call(c, device ? "alz_xxh32_batch_device" : "alz_xxh32_batch", device, a, no_refusal, [] { return (size_t)0; }, [](uint8_t*) { return hipSuccess; },
        [&](const uint8_t* d_src, const alz_stream* d_ranges, uint8_t*, uint32_t* d_out) { return alz_launch_xxh32(c->stream, seed, d_src, d_ranges, a.n, d_out); });
}
int alz_xxh32_batch(alz_ctx* c, uint32_t seed, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    return xxh32_batch(c, false, seed, {n, src_base, src_bytes, ranges, out});
}
int alz_xxh32_batch_device(alz_ctx* c, uint32_t seed, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* ranges, uint32_t* out) {
    return xxh32_batch(c, true, seed, {n, d_src_base, src_bytes, ranges, out});
}
// The range copy of the batched LZ4 / Snappy file layer (alz_xxh32.h): HBM to HBM, one launch for the whole list
int alz_host_range_copy(alz_ctx* c, uint32_t n, alz_copy_range* ranges, const uint8_t* d_src, size_t src_bytes, uint8_t* d_dst, size_t dst_bytes) {
    if (!c || (n && (!ranges || !d_src || !d_dst))) return fail(ALZ_E_INVALID, "alz_host_range_copy: bad argument");
    uint64_t pieces = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!range_ok(ranges[i].src_off, ranges[i].n, src_bytes) || !range_ok(ranges[i].dst_off, ranges[i].n, dst_bytes))
            return fail(ALZ_E_INVALID, "alz_host_range_copy: range %u exceeds its buffer", i);
        ranges[i].first = (uint32_t)pieces;
        pieces += ((uint64_t)ranges[i].n + ALZ_COPY_PIECE - 1) / ALZ_COPY_PIECE;
        if (pieces > 0x7FFFFFFFull) return fail(ALZ_E_UNSUPPORTED, "alz_host_range_copy: more than 2^31 pieces");
    }
    if (pieces == 0) return ALZ_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = grow(c, &c->d_plan, &c->d_plan_cap, (size_t)n * sizeof(alz_copy_range))) return rc;
    hipError_t e = hipMemcpyAsync(c->d_plan, ranges, (size_t)n * sizeof(alz_copy_range), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = alz_launch_range_copy(c->stream, d_src, d_dst, (const alz_copy_range*)c->d_plan, n, (uint32_t)pieces);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(ALZ_E_HIP, "alz_host_range_copy failed: %s", hipGetErrorString(e));
    return ALZ_OK;
}

// Device buffers of one encode call, freed on every exit path
struct EncScratch {
    alz_ctx* c; hipError_t err = hipSuccess;
    explicit EncScratch(alz_ctx* ctx) : c(ctx) {}
    // the context's buffer `k` (alz_ctx::ENC_...), grown to `bytes`; `want` = false leaves it alone (its buffer, if any, stays for a later call).
    // nullptr then, and after a failure: `err` keeps the first one, and nothing more is allocated behind it
    void* get(int k, size_t bytes, bool want = true) {
        if (!want || err != hipSuccess) return nullptr;
        if (bytes < 16) bytes = 16;
        if (c->enc_cap[k] < bytes) {
            if (c->enc_buf[k]) { (void)hipFree(c->enc_buf[k]); c->enc_buf[k] = nullptr; c->enc_cap[k] = 0; }
            err = hipMalloc(&c->enc_buf[k], bytes);
            if (err != hipSuccess) { c->enc_buf[k] = nullptr; return nullptr; }
            c->enc_cap[k] = bytes;
        }
        return c->enc_buf[k];
    }
};
// (alz_encode_seg.h) 1: a small batch of this format is walked speculatively per segment (alz_encode_seg_seq.h), not from synchronisation points
extern "C++" int alz_encode_seg_spec_format(int fmt);
static void release_scratch(alz_ctx* c) {
    for (int k = 0; k < alz_ctx::ENC_SLOTS; k++) { if (c->enc_buf[k]) (void)hipFree(c->enc_buf[k]); c->enc_buf[k] = nullptr; c->enc_cap[k] = 0; }
    const struct { void** buf; size_t* cap; } own[] = {{&c->d_src, &c->d_src_cap}, {&c->d_dst, &c->d_dst_cap}, {&c->d_items, &c->d_items_cap}, {&c->d_pack, &c->d_pack_cap}, {&c->d_plan, &c->d_plan_cap}, {&c->d_bigbuf, &c->d_bigbuf_cap}};
    for (const auto& o : own) { if (*o.buf) (void)hipFree(*o.buf); *o.buf = nullptr; *o.cap = 0; }
}
int alz_ctx_release_scratch(alz_ctx* c) {
    if (!c) return fail(ALZ_E_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    release_scratch(c);
    return ALZ_OK;
}

// FastLZ.CompressHeaderless picks level 2 per source  FastLZ.cs:169-175
static inline bool fastlz_level2(const alz_settings& st, uint32_t src_len) { return src_len >= 0x10000u && st.quality > 4 && st.max_window_bits > 13; }

// The encode of one batch with everything on the device: `streams` (a host table) holds offsets relative to d_src / d_dst, which
// the caller has filled / will read.  `upload(d_src, d_dst)` runs once the arguments are validated and the scratch exists -- the
// host-buffer entry points grow their device buffers and stage their input there (a refused batch never touches the device);
// the device-resident entry point just hands its two pointers over.
// `src_has_slack`: the source buffer has >= 64 readable bytes behind src_bytes (the library's own staging buffer).  A caller's device
// buffer need not: the finder's look-ahead loads read up to 32 bytes past a stream's end, so the streams that end inside the last 64
// bytes of the caller's buffer are copied into scratch with room behind them and searched there (their descriptors -- the device copy
// only -- point at the copy; offsets are differences of device addresses).
// encode_core runs the stages below in turn; what one stage works out for the next travels in these three structs.
namespace {
// One format slot of a batch: ALZ_FMT_COUNT slots for the public formats, one for FastLZ level 2, which has a geometry and a launch of its own, and behind it
// the internal formats of alz_bitlz.h (CRILAYLA, ALLZ), which only alz_bitenc_encode_batch* can name: ALZ_ENCFMT_END in all
struct enc_slot {
    unsigned char* geom = nullptr;                 // alz_encode_geometry's bytes (all zero while the batch has no stream of the slot)
    uint32_t seg_len = 0, seg_kmax = 0;            // the segmented parse + emit (alz_encode_seg.h) takes the slot's launch: segment length and segments per buffer
    bool min_table = false, narrows = false, match = false, mask = false;   // the scratch the slot's kernels need: the min-length table's links, the narrowed links, the match array, the start mask
};
struct enc_batch {
    alz_settings st; alz_lz_properties lz;
    uint32_t cnt[ALZ_ENCFMT_END], off[ALZ_ENCFMT_END];   // per format (slot ALZ_FMT_COUNT stays empty here); a FastLZ list holds the level-1 streams first, then the n_fastlz2 level-2 ones
    std::vector<uint32_t> index; std::vector<uint64_t> pos_off;   // pos_off: where a stream's positions start in the per-position scratch arrays, `total` positions in all
    uint64_t total = 0; uint32_t max_len = 0, n_fastlz2 = 0;
    std::vector<unsigned char> geom_bytes; enc_slot slot[ALZ_ENCFMT_END]; size_t seg_bytes = 0;
    bool any(bool enc_slot::*need) const { for (const enc_slot& s : slot) if (s.*need) return true; return false; }
};
// The device side of one call, shared by its two paths: the buffers `upload` hands over (once), and the streams relocated out of a caller's tail
struct enc_io {
    const std::function<int(const void*&, void*&)>& upload; size_t src_bytes; bool src_has_slack; phase_timer tm;
    const void* d_src = nullptr; void* d_dst = nullptr; bool staged = false;
    std::vector<alz_stream> moved; bool tails_done = false;      // the stream table with the relocated streams' src_off patched (empty: nothing moved)
    int stage() { if (staged) return ALZ_OK; const int rc = upload(d_src, d_dst); staged = rc == ALZ_OK; tm.mark("upload"); return rc; }
};
}
// Stage 1: the settings, then the streams
// (`kinds`: ALZ_FMT_COUNT for the public entry points -- an internal format is an unknown one there --, ALZ_ENCFMT_END for alz_bitenc_encode_batch*' translated table)
static int enc_validate(const alz_settings* settings, uint32_t kinds, uint32_t n, size_t src_bytes, const alz_stream* streams, size_t dst_bytes, alz_settings* out) {
    alz_settings st; if (settings) st = *settings; else { st.quality = 8; st.max_window_bits = 0; st.strategy = 0; st.min_distance = 0; }
    if (st.quality < 0 || st.quality > 15) return fail(ALZ_E_INVALID, "quality %d outside 0..15 (CompressionSettings.cs:38-50)", st.quality);
    if (st.max_window_bits < 0 || st.max_window_bits > 24) return fail(ALZ_E_INVALID, "max_window_bits %d outside 0..24", st.max_window_bits);
    *out = st;
    return validate_streams("", kinds, n, streams, &src_bytes, &dst_bytes, [](uint32_t i, const alz_stream& s) -> int {
        return s.src_len > 0x7FFFFF00u ? fail(ALZ_E_UNSUPPORTED, "stream %u: inputs above 2 GiB are not supported", i) : ALZ_OK;
    });
}
// Stage 2: the streams grouped per format, their places in the per-position arrays, and the geometry of every format slot present
static int enc_geometry(const alz_ctx* c, uint32_t n, const alz_stream* streams, enc_batch* b) {
    const alz_settings& st = b->st;
    group_streams(n, ALZ_ENCFMT_END, [&](uint32_t i) { return streams[i].format; }, b->index, b->off, b->cnt);
    const uint32_t* cnt = b->cnt;
    b->pos_off.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        if (streams[i].format == ALZ_FMT_FASTLZ && fastlz_level2(st, streams[i].src_len)) b->n_fastlz2++;
        b->pos_off[i] = b->total; b->total += ((uint64_t)streams[i].src_len + 16 + 63) & ~63ull;   // 64-aligned: one start-mask word per 64 positions
        if (streams[i].src_len > b->max_len) b->max_len = streams[i].src_len;
    }
    if (b->n_fastlz2)                                        // FastLZ: the level-1 streams first, then the level-2 ones (own geometry, own launch)
        std::stable_partition(b->index.begin() + b->off[ALZ_FMT_FASTLZ], b->index.begin() + b->off[ALZ_FMT_FASTLZ] + cnt[ALZ_FMT_FASTLZ],
                              [&](uint32_t i) { return !fastlz_level2(st, streams[i].src_len); });
    const uint32_t n_fastlz2 = b->n_fastlz2, max_len = b->max_len;
    if (cnt[ALZ_FMT_LZSS] && (!lzss_on_gpu(b->lz) || b->lz.max_distance != (1u << b->lz.window_bits))) return fail(ALZ_E_UNSUPPORTED, "LZSS geometry outside the GPU path");
    b->geom_bytes.resize(ALZ_ENCFMT_END * alz_encode_geom_size());   // (zeros) slot ALZ_FMT_COUNT: FastLZ level 2
    for (int f = 0; f < ALZ_ENCFMT_END; f++) {
        enc_slot& s = b->slot[f];
        void* g = s.geom = b->geom_bytes.data() + f * alz_encode_geom_size();
        const bool lvl2 = f == ALZ_FMT_COUNT;
        if (lvl2 ? !n_fastlz2 : !(cnt[f] - (f == ALZ_FMT_FASTLZ ? n_fastlz2 : 0u))) continue;
        // ALLZ at quality 1: maxChain is 2 and the managed chain table has 1 << min(17 + 1, 19) slots for a window of 1 << 19, so a slot is reused INSIDE
        // maxDistance and GetNext is no longer prev() (LzChainMatchFinder.cs:94-96; alz_encode_geometry's check): what the kernels compute is not what it finds
        if (f == ALZ_ENCFMT_ALLZ && st.quality == 1)
            return fail(ALZ_E_UNSUPPORTED, "ALLZ at quality 1: the managed chain table (2^18 slots) is smaller than the 2^19 window, its links are not prev(): not reproduced on the GPU (every other quality 0..15 is)");
        // aPLib at qualities 1..7: the same table -- 1 << min(17 + floor(sqrt(2 q)), 21) slots -- under a window of 1 << 21.  While no stream of the call is longer
        // than the table no slot is ever reused and the links ARE prev(): the rule is applied per call (variant bit 1 tells alz_encode_geometry that it was)
        int ap_chain_ok = 0;
        if (f == ALZ_ENCFMT_APLIB && st.quality >= 1 && st.quality <= 7) {
            int r = 0; while ((r + 1) * (r + 1) <= 2 * st.quality) r++;
            const uint32_t slots = 1u << (17 + r);
            for (uint32_t i = 0; i < n; i++)
                if (streams[i].format == ALZ_ENCFMT_APLIB && streams[i].src_len > slots)
                    return fail(ALZ_E_UNSUPPORTED, "aPLib at quality %d: stream %u has %u bytes, more than the managed chain table's %u slots (the window is 2^21): its links are not prev() "
                                "beyond that, not reproduced on the GPU (qualities 0 and 8..15 take any length)", st.quality, i, streams[i].src_len, slots);
            ap_chain_ok = 2;
        }
        alz_settings sf = st;
        if (st.max_window_bits != 0 && f != ALZ_FMT_FASTLZ && !lvl2) {
            // CompressionSettings.MaxWindowBits can only WIDEN the finder (windowsBits = max(.., maxWindowBits), maxDistance = max(.., 1 <<
            // maxWindowBits)  MatchFinder/LzChainMatchFinder.cs:69-73): a value within the format's own window changes nothing, and the
            // batch is encoded as with 0.  A larger one lets the managed finder return distances the format cannot store (FastLZ, whose
            // level 2 is selected by it, aside): the caller's own encoder.
            sf.max_window_bits = 0;
            int wb0 = 0;
            if (!alz_encode_geometry(f, &b->lz, &sf, g, &wb0, 0)) return fail(ALZ_E_UNSUPPORTED, "format %d: geometry not supported by the GPU encoder", f);
            if (st.max_window_bits > wb0 || (1ll << st.max_window_bits) > (long long)alz_encode_geom_max_dist(g))
                return fail(ALZ_E_UNSUPPORTED, "format %d: CompressionSettings.MaxWindowBits %d is beyond the format's window (%d bits, distances up to %d): "
                            "the managed finder would return distances the format cannot store", f, st.max_window_bits, wb0, alz_encode_geom_max_dist(g));
        }
        if (!alz_encode_geometry(lvl2 ? ALZ_FMT_FASTLZ : f, &b->lz, &sf, g, nullptr, ((lvl2 || (f > ALZ_FMT_COUNT && c->exact)) ? 1 : 0) | ap_chain_ok))   // (CRILAYLA, ALLZ, aPLib: 1 = their lone-lane emitters)
            return fail(ALZ_E_UNSUPPORTED, "format %d: geometry not supported by the GPU encoder", lvl2 ? ALZ_FMT_FASTLZ : f);
        s.min_table = alz_encode_geom_min_table(g);
        s.narrows = alz_encode_geom_narrows(g);
        s.match = alz_encode_geom_needs_match(lvl2 ? ALZ_FMT_FASTLZ : f, g);
        s.mask = alz_encode_format_needs_mask(lvl2 ? ALZ_FMT_FASTLZ : f);
        // a batch of few buffers of a flag-bit format: parse and emitter over segments (alz_encode_seg.h) -- behind kernel B and the roles walk
        uint32_t seg_hist = 0;
        if (!lvl2 && !c->exact && c->variant == 0 && alz_encode_segmented(f, g, cnt[f], max_len, c->seg_max_streams, &s.seg_len, &s.seg_kmax, &seg_hist)) {
            s.match = s.mask = true;
            size_t ab = 0; (void)alz_encode_aseg(g, cnt[f], max_len, nullptr, nullptr, nullptr, nullptr, &ab);
            const size_t sb = ((alz_encode_seg_bytes(cnt[f], s.seg_kmax, seg_hist) + 255) & ~(size_t)255) + ab; if (sb > b->seg_bytes) b->seg_bytes = sb;
        }
    }
    return ALZ_OK;
}
// Stage 3: a handful of big streams: each of them on the whole GPU (alz_encode_big.h)?  true: yes, with *scratch the bytes that path needs.
// As in the decoder (plan_create): one after the other on the whole GPU while that beats side by side with a workgroup + a wavefront
// each -- measured at quality 0-8 on Test.bmp (tools/mid_batch_encode.py): ~0.10 ms + 0.10 ms per MiB on the whole GPU, ~22 ms per MiB of the LONGEST buffer side by side.
static bool enc_takes_big_path(const alz_ctx* c, const enc_batch& b, uint32_t n, const alz_stream* streams, size_t* scratch) {
    const uint32_t* cnt = b.cnt; const uint32_t max_len = b.max_len;
    if (!(n <= ALZ_BIG_MAX_STREAMS && c->big_min != 0xFFFFFFFFu && !c->exact && c->variant == 0)) return false;
    // (from 8 KiB on -- not the decoder's 24 KiB: ONE buffer of 8 KiB takes 0.08 ms of kernels this way and 0.22 through the batch pipeline, of
    // 64 KiB 0.10 against 1.6, tools/single_encode_sizes.py; a threshold the caller has set below that is the caller's)
    const uint32_t enc_min = c->big_min < 8192u ? c->big_min : 8192u;
    bool all = true; size_t sb = 0;
    double t_big = 0, t_side = 0;
    const bool q0 = b.st.quality == 0;                                        // (no narrowing behind kernel A, one candidate per position in kernel B: 8 x 1 MB 0.99 one by one / 0.68)
    for (uint32_t i = 0; all && i < n; i++) {
        const void* g = b.slot[streams[i].format].geom;
        all = streams[i].format != ALZ_FMT_FASTLZ && alz_encode_big_eligible((int)streams[i].format, g, &streams[i], enc_min);
        if (all) { const size_t sbi = alz_encode_big_scratch_bytes((int)streams[i].format, g, &streams[i]); if (sbi > sb) sb = sbi; }
        const double mib = streams[i].src_len / 1048576.0;
        // (round 6, 2-32 x 1 MiB of Test.bmp one by one, ms per MiB: LZ4 blocks / LZO -- 64 KiB windows -- 0.32 at quality 0 and 0.80 at quality 8, LZ11 / LZ40 0.21 / 0.37)
        const bool wide = alz_encode_geom_max_dist(g) > 8192, l11 = streams[i].format == ALZ_FMT_LZ11 || streams[i].format == ALZ_FMT_LZ40;
        const double rate = wide ? (q0 ? 0.22 : 0.70) : (l11 && !q0) ? 0.27 : 0.10;
        t_big += 0.10 + rate * mib; if (22.0 * mib > t_side) t_side = 22.0 * mib;
    }
    // (side by side is no longer one wavefront per buffer where the segmented parse + emit takes the launch, alz_encode_seg.h: what is left of the longest
    // buffer's serial time is kernel A -- over segments too, for these few buffers: ~0.9 ms per MiB; one workgroup per buffer where that does not apply: 2.2 --
    // + ~0.14 ms of small kernels per format + ~0.08 ms per MiB of the whole call.  tools/mid_batch_encode.py with ALZ_MID_BIG=on / off,
    // profiles/r05_mid_big_vs_seg.txt: 4 x 256 KiB at quality 8 0.47 ms one by one against 0.42, 8 x 1 MB 1.66 / 1.73, 16 x 1 MB 3.33 / 2.18)
    {
        bool seg_all = true, aseg_all = true, spec_any = false, wide_any = false; int nf = 0; double mib_all = 0;
        for (int f = 0; f < ALZ_FMT_COUNT; f++) if (cnt[f]) {
            nf++; seg_all = seg_all && b.slot[f].seg_len != 0; spec_any = spec_any || alz_encode_seg_spec_format(f);
            wide_any = wide_any || alz_encode_geom_max_dist(b.slot[f].geom) > 8192;
            aseg_all = aseg_all && alz_encode_aseg(b.slot[f].geom, cnt[f], max_len, nullptr, nullptr, nullptr, nullptr, nullptr);
        }
        for (uint32_t i = 0; i < n; i++) mib_all += streams[i].src_len / 1048576.0;
        // (the formats of the speculative walk -- alz_encode_seg_seq.h -- have one serial step per segment of the longest buffer behind that, and the 64 KiB windows above quality 0 their
        // words / narrowing passes: ~0.4 / 2.0 ms per MiB; 2 / 4 / 8 / 16 x 1 MiB at the end of round 6, ms, one by one | side by side: LZ4 blocks at quality 0 0.65 / 1.28 / 2.53 / 5.09 |
        // 0.99 / 1.03 / 1.11 / 1.60, at quality 8 1.61 / 3.19 / 6.39 / 12.8 | 2.93 / 3.06 / 3.43 / 4.63; LZ11 at quality 0 0.42 / 0.84 / 1.64 / 3.27 | 0.72 / 0.79 / 0.90 / 1.42, at quality 8
        // 0.76 / 1.47 / 2.92 / 5.89 | 1.65 / 1.84 / 2.07 / 2.95)
        const double t_spec = spec_any ? ((wide_any && !q0) ? 2.0 : 0.4) : 0.0;
        if (seg_all) { const double t_seg = 0.14 * nf + ((aseg_all ? (q0 ? 0.45 : 0.9) : 2.2) + t_spec) * (max_len / 1048576.0) + (q0 ? 0.03 : 0.08) * mib_all; if (t_seg < t_side) t_side = t_seg; }
    }
    *scratch = sb;
    return all && t_big < t_side;
}
// Stage 4: the streams whose look-ahead would leave the caller's source buffer (`src_has_slack`, below) are copied into scratch with room behind
// them, and their descriptors -- in `moved`, the table the device gets -- point at the copy.  Once per call, whichever path asks first.
static hipError_t enc_relocate_tails(alz_ctx* c, enc_io& io, uint32_t n, const alz_stream* streams) {
    if (io.src_has_slack || io.tails_done) return hipSuccess;
    io.tails_done = true;
    // (a CRILAYLA stream is never searched where it lies: the batch path reverses it into scratch of its own, with room behind it)
    auto in_tail = [&](const alz_stream& s) { return s.format != ALZ_ENCFMT_CRILAYLA && s.src_off + s.src_len + 64 > io.src_bytes; };
    auto room = [](const alz_stream& s) { return ((size_t)s.src_len + 64 + 63) & ~(size_t)63; };
    size_t bytes = 0; for (uint32_t i = 0; i < n; i++) if (in_tail(streams[i])) bytes += room(streams[i]);
    if (!bytes) return hipSuccess;
    EncScratch sc(c);
    uint8_t* to = (uint8_t*)sc.get(alz_ctx::ENC_TAIL, bytes);
    if (!to) return sc.err;
    io.moved.assign(streams, streams + n);
    for (uint32_t i = 0; i < n; i++) {
        if (!in_tail(streams[i])) continue;
        if (streams[i].src_len)
            if (hipError_t e = hipMemcpyAsync(to, (const uint8_t*)io.d_src + streams[i].src_off, streams[i].src_len, hipMemcpyDeviceToDevice, c->stream)) return e;
        io.moved[i].src_off = (uint64_t)(uintptr_t)to - (uint64_t)(uintptr_t)io.d_src;
        to += room(streams[i]);
    }
    return hipSuccess;
}
// Stage 5: every stream on the whole GPU, one after the other.  *taken = false: a stream was declined (too many positions that need an exact
// second search) and nothing has been delivered: the batch path below encodes the call.
static int enc_big_path(alz_ctx* c, const enc_batch& b, enc_io& io, uint32_t n, const alz_stream* streams, size_t sb, alz_result* results, alz_encode_aux* aux, bool* taken) {
    EncScratch sc(c); *taken = false;
    // what travels back: per stream its result, its section offsets and the path's 16 control words -- one block, one copy
    const size_t out_one = sizeof(alz_result) + sizeof(alz_encode_aux) + 16 * sizeof(uint32_t), sb_al = (sb + 255) & ~(size_t)255;
    void* d_big = sc.get(alz_ctx::ENC_BIG, sb_al + (size_t)n * out_one + 64);
    if (sc.err != hipSuccess) return fail(ALZ_E_NOMEM, "encoder scratch allocation failed: %s", hipGetErrorString(sc.err));
    uint8_t* d_out = (uint8_t*)d_big + sb_al;
    alz_result* d_results = (alz_result*)d_out;
    alz_encode_aux* d_aux = (alz_encode_aux*)(d_out + (size_t)n * sizeof(alz_result));
    uint32_t* d_ctl = (uint32_t*)(d_out + (size_t)n * (sizeof(alz_result) + sizeof(alz_encode_aux)));
    int rc = io.stage();
    if (rc) return rc;
    std::vector<uint8_t> hout((size_t)n * out_one);
    rc = launch_bracket(c, "alz_encode_batch", [] { return hipSuccess; },
        [&] {
            hipError_t e = enc_relocate_tails(c, io, n, streams);        // (between the events, where this path's copies have always been)
            const alz_stream* table = io.moved.empty() ? streams : io.moved.data();
            for (uint32_t i = 0; i < n && e == hipSuccess; i++)
                e = alz_launch_encode_big((int)table[i].format, c->stream, io.d_src, io.d_dst, &table[i], d_results + i, d_aux + i, d_big, d_ctl + 16 * (size_t)i, b.slot[table[i].format].geom);
            return e;
        },
        [&] { return hipMemcpyAsync(hout.data(), d_out, hout.size(), hipMemcpyDeviceToHost, c->stream); });
    if (rc) return rc;
    io.tm.mark("kernels (big streams)");
    const alz_encode_aux* haux = (const alz_encode_aux*)(hout.data() + (size_t)n * sizeof(alz_result));
    const uint32_t* hctl = (const uint32_t*)(hout.data() + (size_t)n * (sizeof(alz_result) + sizeof(alz_encode_aux)));
    for (uint32_t i = 0; i < n; i++) if (hctl[16 * (size_t)i] != 0u) return ALZ_OK;
    c->big_enc_launches += n;
    memcpy(results, hout.data(), (size_t)n * sizeof(alz_result));
    for (uint32_t i = 0; i < n; i++) if (aux) aux[i] = haux[i];
    *taken = true;
    return ALZ_OK;
}
// Stage 6: the batch pipeline, one launch per format slot present
static int enc_batch_path(alz_ctx* c, const enc_batch& b, enc_io& io, uint32_t n, const alz_stream* streams, alz_result* results, alz_encode_aux* aux) {
    const uint32_t* cnt = b.cnt; const uint64_t total = b.total;
    const bool any_min = b.any(&enc_slot::min_table), any_match = b.any(&enc_slot::match), any_mask = b.any(&enc_slot::mask), any_narrow = b.any(&enc_slot::narrows);
    // (kernel A keeps its hash table in LDS: no per-stream tables in HBM, nothing that bounds the streams of a launch but the grid:
    // a launch carries the stream in gridDim.y; 70 000 went through on this runtime, the cap is caution)
    const uint32_t CH = 65535u;
    EncScratch sc(c);
    alz_stream* d_streams = (alz_stream*)sc.get(alz_ctx::ENC_STREAMS, (size_t)n * sizeof(alz_stream));
    alz_result* d_results = (alz_result*)sc.get(alz_ctx::ENC_RESULTS, (size_t)n * sizeof(alz_result));
    alz_encode_aux* d_aux = (alz_encode_aux*)sc.get(alz_ctx::ENC_AUX, (size_t)n * sizeof(alz_encode_aux));
    uint32_t* d_index = (uint32_t*)sc.get(alz_ctx::ENC_INDEX, (size_t)n * sizeof(uint32_t));
    uint64_t* d_pos = (uint64_t*)sc.get(alz_ctx::ENC_POS, (size_t)n * sizeof(uint64_t));
    int* d_prev4 = (int*)sc.get(alz_ctx::ENC_PREV4, (size_t)total * sizeof(int) + 256);   // (+ slack: the look-ahead of the fused parse kernel reads a link of an empty last stream)
    int* d_prevm = (int*)sc.get(alz_ctx::ENC_PREVM, (size_t)total * sizeof(int) + 256, any_min);   // the min-length table's links
    void* d_match = sc.get(alz_ctx::ENC_MATCH, (size_t)total * 4 + 64, any_match);   // one 32-bit entry per position (alz_encode.hip: mentry); not when every launch searches inside its parse + emit kernel
    void* d_side = sc.get(alz_ctx::ENC_SIDE, (size_t)total * 2 + 64, cnt[ALZ_FMT_YAY0] || cnt[ALZ_FMT_MIO0] || cnt[ALZ_FMT_SMSR00]);   // section buffers
    void* d_mask = sc.get(alz_ctx::ENC_MASK, (size_t)total / 8 + 64, any_mask);          // a bit per position: the start mask of enc_roles_kernel, for the formats whose emitter is a kernel of its own
    uint32_t* d_sel = (uint32_t*)sc.get(alz_ctx::ENC_SEL, ((size_t)4 * n + 128) * sizeof(uint32_t), any_match);     // which kernel B per stream (enc_probe_kernel); behind it the two lists of enc_scan_select_kernel
    int* d_narrow = (int*)sc.get(alz_ctx::ENC_NARROW, (size_t)total * sizeof(int) + 256, any_narrow);   // the links of the finder's own hash width, narrowed from 15-bit ones (enc_narrow_kernel)
    void* d_seg = sc.get(alz_ctx::ENC_SEG, b.seg_bytes, b.seg_bytes != 0);                              // segment records of alz_encode_seg.h
    // CRILAYLA: every stream's reversed copy, 64 readable bytes behind each, in front of them the streams' own source offsets (what enc_bits_reverse_kernel reads from)
    auto rev_room = [](const alz_stream& s) { return ((size_t)s.src_len + 64 + 63) & ~(size_t)63; };
    const size_t rev_head = ((size_t)n * sizeof(uint64_t) + 255) & ~(size_t)255;
    size_t rev_bytes = rev_head; std::vector<uint64_t> orig_off;
    if (cnt[ALZ_ENCFMT_CRILAYLA]) for (uint32_t i = 0; i < n; i++) if (streams[i].format == ALZ_ENCFMT_CRILAYLA) rev_bytes += rev_room(streams[i]);
    uint8_t* d_rev = (uint8_t*)sc.get(alz_ctx::ENC_REV, rev_bytes, cnt[ALZ_ENCFMT_CRILAYLA] != 0);
    const uint64_t* d_orig = (const uint64_t*)d_rev;
    if (sc.err != hipSuccess) return fail(ALZ_E_NOMEM, "encoder scratch allocation failed: %s", hipGetErrorString(sc.err));
    io.tm.mark("validate + allocate");
    int rc = io.stage();
    if (rc) return rc;
    std::vector<alz_encode_aux> haux(n);
    const alz_encode_side side_q = { c->aux[0], c->fork, c->join[1] };      // (the scan streams' kernel runs beside the others: alz_launch_encode)
    rc = launch_bracket(c, "alz_encode_batch",
        [&] {   // (the tables are read out of `io.moved`, `b` and the caller's table: the bracket waits for the copies)
            hipError_t e = enc_relocate_tails(c, io, n, streams);
            if (e == hipSuccess && d_rev) {     // (the device copy of the descriptors points at the reversed bytes, as it does at a relocated tail)
                if (io.moved.empty()) io.moved.assign(streams, streams + n);
                orig_off.resize(n);
                uint8_t* to = d_rev + rev_head;
                for (uint32_t i = 0; i < n; i++) {
                    orig_off[i] = io.moved[i].src_off;
                    if (streams[i].format != ALZ_ENCFMT_CRILAYLA) continue;
                    io.moved[i].src_off = (uint64_t)(uintptr_t)to - (uint64_t)(uintptr_t)io.d_src;
                    to += rev_room(streams[i]);
                }
                e = hipMemcpyAsync(d_rev, orig_off.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
            }
            if (e == hipSuccess) e = hipMemcpyAsync(d_streams, io.moved.empty() ? streams : io.moved.data(), (size_t)n * sizeof(alz_stream), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_index, b.index.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(d_pos, b.pos_off.data(), (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemsetAsync(d_results, 0xFF, (size_t)n * sizeof(alz_result), c->stream);
            if (e == hipSuccess) e = hipMemsetAsync(d_aux, 0, (size_t)n * sizeof(alz_encode_aux), c->stream);
            if (e == hipSuccess && any_mask) e = hipMemsetAsync(d_mask, 0, (size_t)total / 8 + 64, c->stream);
            return e;
        },
        [&] {   // table resets + the encode kernels
            for (int f = 0; f < ALZ_ENCFMT_END; f++) {
                const bool lvl2 = f == ALZ_FMT_COUNT;
                const int fmt = lvl2 ? ALZ_FMT_FASTLZ : f;
                const uint32_t first = b.off[fmt] + (lvl2 ? cnt[fmt] - b.n_fastlz2 : 0u);
                const uint32_t count = lvl2 ? b.n_fastlz2 : cnt[f] - (f == ALZ_FMT_FASTLZ ? b.n_fastlz2 : 0u);
                const enc_slot& s = b.slot[f];
                for (uint32_t done = 0; done < count; done += CH) {
                    const uint32_t k = count - done < CH ? count - done : CH;
                    if (f == ALZ_ENCFMT_CRILAYLA)                                  // the finder runs over the reversed source  CRILAYLA.cs:204-206
                        if (const hipError_t er = alz_launch_encode_reverse(c->stream, io.d_src, d_rev, d_streams, d_orig, d_index + first + done, k, b.max_len)) return er;
                    // (positional on purpose: the prototype lives in alz_internal.h, which the decode counters are hashed over -- a struct in its place belongs to the change that next re-profiles the decoder)
                    const hipError_t e = alz_launch_encode(fmt, c->stream, io.d_src, io.d_dst, d_streams, d_index + first + done, k, b.max_len, d_prev4, d_prevm, d_narrow,
                                          d_match, d_pos, d_side, d_mask, d_results, d_aux, s.geom, d_sel, n, s.seg_len ? d_seg : nullptr, s.seg_len, s.seg_kmax, (c->exact || c->variant != 0) ? 2 : c->scan_mode, c->d_big_accepted ? c->d_big_accepted + 1 : nullptr, &side_q);
                    if (e != hipSuccess) return e;
                    if (s.seg_len) c->seg_enc_launches++;
                }
            }
            return hipSuccess;
        },
        [&] { const hipError_t e = hipMemcpyAsync(results, d_results, (size_t)n * sizeof(alz_result), hipMemcpyDeviceToHost, c->stream);
              return e == hipSuccess ? hipMemcpyAsync(haux.data(), d_aux, (size_t)n * sizeof(alz_encode_aux), hipMemcpyDeviceToHost, c->stream) : e; });
    if (rc) return rc;
    io.tm.mark("kernels");
    for (uint32_t i = 0; i < n; i++) if (aux) aux[i] = haux[i];
    return ALZ_OK;
}
static int encode_core(alz_ctx* c, const alz_lz_properties* props, const alz_settings* settings, uint32_t n, size_t src_bytes, const alz_stream* streams,
                       size_t dst_bytes, alz_result* results, alz_encode_aux* aux, const std::function<int(const void*&, void*&)>& upload, bool src_has_slack = true,
                       uint32_t kinds = ALZ_FMT_COUNT) {
    enc_batch b; int rc;
    if ((rc = enc_validate(settings, kinds, n, src_bytes, streams, dst_bytes, &b.st))) return rc;
    b.lz = effective_lz(props);
    enc_io io{upload, src_bytes, src_has_slack, phase_timer("alz_encode_batch")};
    if ((rc = enc_geometry(c, n, streams, &b))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // A stream the whole-GPU path declines sends the whole call through the batch pipeline: in this same invocation, over the source staged once
    size_t big_scratch = 0; bool taken = false;
    if (enc_takes_big_path(c, b, n, streams, &big_scratch) && ((rc = enc_big_path(c, b, io, n, streams, big_scratch, results, aux, &taken)) || taken)) return rc;
    return enc_batch_path(c, b, io, n, streams, results, aux);
}

int alz_encode_batch(alz_ctx* c, const alz_lz_properties* props, const alz_settings* settings, uint32_t n, const uint8_t* src_base,
                     size_t src_bytes, const alz_stream* streams, uint8_t* dst_base, size_t dst_bytes, alz_result* results, alz_encode_aux* aux) {
    if (!c || (n && (!streams || !results || !dst_base))) return fail(ALZ_E_INVALID, "alz_encode_batch: bad argument");
    if (n == 0) return ALZ_OK;
    const int rc = encode_core(c, props, settings, n, src_bytes, streams, dst_bytes, results, aux, [&](const void*& ds, void*& dd) {
        const int r = stage_source(c, src_base, src_bytes, true, dst_bytes);
        ds = c->d_src; dd = c->d_dst;
        return r;
    });
    return rc ? rc : download_outputs(c, n, streams, results, dst_base, true);
}

// The same with the raw buffers already in HBM and the compressed streams left there (alz_stream offsets are relative to the two
// device pointers): what a caller that produces its input on the device uses, and what a benchmark times -- kernels, no PCIe.
int alz_encode_batch_device(alz_ctx* c, const alz_lz_properties* props, const alz_settings* settings, uint32_t n, const void* d_src_base,
                            size_t src_bytes, const alz_stream* streams, void* d_dst_base, size_t dst_bytes, alz_result* results, alz_encode_aux* aux) {
    if (!c || (n && (!streams || !results || !d_src_base || !d_dst_base))) return fail(ALZ_E_INVALID, "alz_encode_batch_device: bad argument");
    if (n == 0) return ALZ_OK;
    return encode_core(c, props, settings, n, src_bytes, streams, dst_bytes, results, aux,
                       [&](const void*& ds, void*& dd) { ds = d_src_base; dd = d_dst_base; return (int)ALZ_OK; }, false);
}

// ---------------------------------------------------------------- CRILAYLA / ALLZ bodies written (alz_encode.hip): CompressHeaderless of the two classes
// streams[i].format is an alz_bitlz_kind; the table the encoder sees names the internal formats behind the public enum.  A lone large buffer goes
// through the batch pipeline like any other (no whole-GPU path, no segments: the two formats have rows without them in ALZ_ENC_PATHS).
size_t alz_bitenc_bound(uint32_t kind, size_t src_len) {
    // CRILAYLA: nine bits per literal; a match (16 bits for three bytes, 14 + 10 + 8 per 255 further ones) is never more than its bytes as literals.
    if (kind == ALZ_BITLZ_CRILAYLA) return (src_len * 9 + 7) / 8;
    // ALLZ: at most src_len / 3 + 1 units of [run?][match].  WriteALFlag(start, v) writes 2 * bits - start + 1 bits with bits <= max(start, bitlen(v) + 1):
    // at most 39 for a distance or a length (v < 2^19, start <= 24), at most 28 + 2 * bitlen(run) for a run, and the bit lengths of all runs add up to
    // no more than their bytes.  So 1 + 28 + 39 + 39 = 107 bits per unit, 2 * src_len bits for the runs' lengths, the runs themselves and the last byte.
    if (kind == ALZ_BITLZ_ALLZ) return src_len + src_len / 4 + 14 * (src_len / 3 + 1) + 2;
    return 0;
}

static int bitenc_batch(alz_ctx* c, bool device, const alz_settings* settings, uint32_t n, const void* src_base, size_t src_bytes, const alz_stream* streams,
                        void* dst_base, size_t dst_bytes, alz_result* results) {
    const char* what = device ? "alz_bitenc_encode_batch_device" : "alz_bitenc_encode_batch";
    if (!c || (n && (!streams || !results || !dst_base || (device && !src_base)))) return fail(ALZ_E_INVALID, "%s: bad argument", what);
    if (n == 0) return ALZ_OK;
    // (the finder's settings: what enc_validate lets through, less the two that would make the managed finder return what neither format can store)
    if (settings && settings->max_window_bits != 0) return fail(ALZ_E_UNSUPPORTED, "%s: max_window_bits %d: CRILAYLA and ALLZ are written at their own windows only", what, settings->max_window_bits);
    if (settings && settings->min_distance != 0) return fail(ALZ_E_UNSUPPORTED, "%s: min_distance %d: CRILAYLA and ALLZ are written at their own minimum distances only", what, settings->min_distance);
    std::vector<alz_stream> table(streams, streams + n);
    for (uint32_t i = 0; i < n; i++) {
        alz_stream& s = table[i];
        if (s.format >= ALZ_BITLZ_COUNT) return fail(ALZ_E_INVALID, "%s: stream %u: unknown format / kind %u", what, i, s.format);
        if (s.format == ALZ_BITLZ_ALLZ) {
            if ((s.aux0 & 0xFFu) > 24u || ((s.aux0 >> 8) & 0xFFu) > 24u || ((s.aux0 >> 16) & 0xFFu) > 24u || (s.aux0 >> 24))
                return fail(ALZ_E_INVALID, "%s: stream %u: ALLZ start bits 0x%x outside 0..24 each", what, i, s.aux0);
            if (s.src_len > 0x40000000u) return fail(ALZ_E_UNSUPPORTED, "%s: stream %u: ALLZ sources above 0x40000000 bytes are not supported (WriteALFlag's int sums)", what, i);
        }
        s.format = s.format == ALZ_BITLZ_CRILAYLA ? (uint32_t)ALZ_ENCFMT_CRILAYLA : (uint32_t)ALZ_ENCFMT_ALLZ;
    }
    if (device)
        return encode_core(c, nullptr, settings, n, src_bytes, table.data(), dst_bytes, results, nullptr,
                           [&](const void*& ds, void*& dd) { ds = src_base; dd = dst_base; return (int)ALZ_OK; }, false, ALZ_ENCFMT_END);
    const int rc = encode_core(c, nullptr, settings, n, src_bytes, table.data(), dst_bytes, results, nullptr, [&](const void*& ds, void*& dd) {
        const int r = stage_source(c, (const uint8_t*)src_base, src_bytes, true, dst_bytes);
        ds = c->d_src; dd = c->d_dst;
        return r;
    }, true, ALZ_ENCFMT_END);
    return rc ? rc : download_outputs(c, n, streams, results, (uint8_t*)dst_base, true);
}
int alz_bitenc_encode_batch(alz_ctx* c, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                            uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return bitenc_batch(c, false, settings, n, src_base, src_bytes, streams, dst_base, dst_bytes, results);
}
int alz_bitenc_encode_batch_device(alz_ctx* c, const alz_settings* settings, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                   uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return bitenc_batch(c, true, settings, n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results);
}

// ---------------------------------------------------------------- aPLib's body written (alz_encode.hip): aPLib.CompressHeaderless  Formats/Common/aPLib.cs:183-286
// Every stream is an aPLib body to be: format, aux0, aux1 and decom_len are ignored, the table the encoder sees names the third internal format.  A lone large
// buffer goes through the batch pipeline like any other (its row in ALZ_ENC_PATHS has no whole-GPU path and no segments).
size_t alz_apenc_bound(size_t src_len) {
    // Literals only is the worst case: source[0], then a bit and a byte per further byte, the end marker's three bits and its byte -- src_len + 1 bytes and
    // src_len + 2 bits.  No other token costs more than 9 bits per byte it covers: a one-byte match 7; a short block 11 for two; a repeat 4 + 2 (bitlen(L) - 1) for
    // L >= 2; a normal block 2 + gamma(high) + 8 + gamma(L - delta) against the minimum length of the set its distance falls in: 14 bits for two bytes at 0x80,
    // at most 20 for three up to 0xFFF, 24 for four up to 0x3FFF, 28 for five, 34 for six, 38 for seven, 40 for eight at the far end; a longer match adds two bits
    // each time L - delta doubles.
    return src_len ? src_len + 1 + (src_len + 2 + 7) / 8 : 0;
}

static int apenc_batch(alz_ctx* c, bool device, const alz_settings* settings, uint32_t n, const void* src_base, size_t src_bytes, const alz_stream* streams,
                       void* dst_base, size_t dst_bytes, alz_result* results) {
    const char* what = device ? "alz_apenc_encode_batch_device" : "alz_apenc_encode_batch";
    if (!c || (n && (!streams || !results || !dst_base || (device && !src_base)))) return fail(ALZ_E_INVALID, "%s: bad argument", what);
    if (n == 0) return ALZ_OK;
    if (settings && (settings->quality < 0 || settings->quality > 15)) return fail(ALZ_E_INVALID, "%s: quality %d outside 0..15 (CompressionSettings.cs:38-50)", what, settings->quality);
    // (the finder's settings: what enc_validate lets through, less the two that would make the managed finder return what the format cannot store)
    if (settings && settings->max_window_bits != 0) return fail(ALZ_E_UNSUPPORTED, "%s: max_window_bits %d: aPLib is written at its own window only", what, settings->max_window_bits);
    if (settings && settings->min_distance != 0) return fail(ALZ_E_UNSUPPORTED, "%s: min_distance %d: aPLib is written at its own minimum distance only", what, settings->min_distance);
    std::vector<alz_stream> table(streams, streams + n);
    for (uint32_t i = 0; i < n; i++) {
        alz_stream& s = table[i];
        if (s.src_len == 0) return fail(ALZ_E_INVALID, "%s: stream %u: an empty source (the managed code throws on source[0]  aPLib.cs:191)", what, i);
        if (s.src_len > 0x40000000u) return fail(ALZ_E_UNSUPPORTED, "%s: stream %u: sources above 0x40000000 bytes are not supported", what, i);
        s.format = (uint32_t)ALZ_ENCFMT_APLIB; s.aux0 = s.aux1 = 0; s.decom_len = 0;
    }
    if (device)
        return encode_core(c, nullptr, settings, n, src_bytes, table.data(), dst_bytes, results, nullptr,
                           [&](const void*& ds, void*& dd) { ds = src_base; dd = dst_base; return (int)ALZ_OK; }, false, ALZ_ENCFMT_END);
    const int rc = encode_core(c, nullptr, settings, n, src_bytes, table.data(), dst_bytes, results, nullptr, [&](const void*& ds, void*& dd) {
        const int r = stage_source(c, (const uint8_t*)src_base, src_bytes, true, dst_bytes);
        ds = c->d_src; dd = c->d_dst;
        return r;
    }, true, ALZ_ENCFMT_END);
    return rc ? rc : download_outputs(c, n, streams, results, (uint8_t*)dst_base, true);
}
int alz_apenc_encode_batch(alz_ctx* c, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results) {
    return apenc_batch(c, false, settings, n, src_base, src_bytes, streams, dst_base, dst_bytes, results);
}
int alz_apenc_encode_batch_device(alz_ctx* c, const alz_settings* settings, uint32_t n, const uint8_t* d_src_base, size_t src_bytes, const alz_stream* streams,
                                  uint8_t* d_dst_base, size_t dst_bytes, alz_result* results) {
    return apenc_batch(c, true, settings, n, d_src_base, src_bytes, streams, d_dst_base, dst_bytes, results);
}

// ---------------------------------------------------------------- multi-GPU: one batch over several contexts
// Decode cost per output byte of a format relative to the fastest one (x64; from the measured per-format rates, docs/EXPERIMENTS.md 4.4)
static uint32_t format_weight(uint32_t fmt) {
    switch (fmt) {
    case ALZ_FMT_YAY0: return 55;
    case ALZ_FMT_YAZ0: case ALZ_FMT_LZ02: case ALZ_FMT_LZ11: case ALZ_FMT_LZ40: return 64;
    case ALZ_FMT_MIO0: case ALZ_FMT_SMSR00: return 78;
    case ALZ_FMT_LZSS: case ALZ_FMT_LZ10: case ALZ_FMT_CLZ0: case ALZ_FMT_CNS: case ALZ_FMT_LZHUDSON: case ALZ_FMT_LZSHREK: return 83;
    case ALZ_FMT_CNX2: case ALZ_FMT_HIG: case ALZ_FMT_PRS_BE: case ALZ_FMT_PRS_LE: case ALZ_FMT_LZ4_BLOCK: case ALZ_FMT_FASTLZ: case ALZ_FMT_WFLZ: case ALZ_FMT_WFLZ_BE: return 109;
    case ALZ_FMT_BLZ: case ALZ_FMT_REFPACK: case ALZ_FMT_SNAPPY_RAW: return 140;
    default: return 171;                                     // LZO
    }
}

int alz_partition_batch(uint32_t n, const alz_stream* streams, uint32_t n_parts, uint32_t* part_of, uint64_t* part_cost) {
    if ((n && (!streams || !part_of)) || n_parts == 0) return fail(ALZ_E_INVALID, "alz_partition_batch: bad argument");
    std::vector<uint64_t> cost(n), load(n_parts, 0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t f = streams[i].format < ALZ_FMT_COUNT ? streams[i].format : 0;
        const uint64_t out = streams[i].decom_len && streams[i].decom_len < streams[i].dst_cap ? streams[i].decom_len : streams[i].dst_cap;
        cost[i] = (out + 4096) * format_weight(f);           // (+ a fixed share: a wave per stream, header / tail handling)
    }
    lpt_deal(n, n_parts, [&](uint32_t i) { return cost[i]; }, part_of, load.data());
    if (part_cost) for (uint32_t q = 0; q < n_parts; q++) part_cost[q] = load[q];
    return ALZ_OK;
}

struct in_seg { uint64_t dev; const uint8_t* host; uint32_t len; };
// packed device range <- scattered host ranges (segments sorted by device offset), window by window through the pinned buffers
static int upload_segs(alz_ctx* c, void* d_base, const std::vector<in_seg>& segs, uint64_t total) {
    if (segs.empty() || total == 0) return ALZ_OK;
    if (ensure_pinned(c) != ALZ_OK) {
        for (const in_seg& g : segs) if (g.len) HIP_TRY(hipMemcpyAsync((uint8_t*)d_base + g.dev, g.host, g.len, hipMemcpyHostToDevice, c->stream));
        return ALZ_OK;
    }
    const uint64_t W = c->pin_cap;
    size_t first = 0; int rcp;
    for (uint64_t a = 0, w = 0; a < total; a += W, w++) {
        const int k = (int)(w & 1);
        const uint64_t b = a + W < total ? a + W : total;
        if ((rcp = pin_wait(c, k))) return rcp;
        while (first < segs.size() && segs[first].dev + segs[first].len <= a) first++;
        c->jobs.clear();
        for (size_t i = first; i < segs.size() && segs[i].dev < b; i++) {
            const uint64_t s0 = segs[i].dev > a ? segs[i].dev : a, s1 = segs[i].dev + segs[i].len < b ? segs[i].dev + segs[i].len : b;
            if (s1 > s0) add_copy(c->jobs, (uint8_t*)c->pin[k] + (s0 - a), segs[i].host + (s0 - segs[i].dev), s1 - s0);
        }
        c->pool->run(c->jobs);
        HIP_TRY(hipMemcpyAsync((uint8_t*)d_base + a, c->pin[k], b - a, hipMemcpyHostToDevice, c->stream));
        if ((rcp = pin_mark(c, k))) return rcp;
    }
    return ALZ_OK;
}

// One context's share of a batch: its streams are packed into device buffers of their own (16-byte aligned inputs, 256-byte
// aligned outputs), so every device receives and returns only the bytes of its share.  `src_slack`: bytes kept free behind every input;
// `lz4_history`: an LZ4 block's history (aux0 bytes) gets room in front of its 256-aligned output slot.
namespace { struct share_layout { std::vector<alz_stream> ds; std::vector<in_seg> ins; uint64_t so = 0, dof = 0; }; }
static share_layout pack_share(const std::vector<uint32_t>& idx, const uint8_t* src_base, const alz_stream* streams, uint32_t src_slack, bool lz4_history) {
    share_layout L; L.ds.reserve(idx.size()); L.ins.reserve(idx.size());
    for (uint32_t i : idx) {
        alz_stream st = streams[i];
        L.ins.push_back(in_seg{L.so, src_base + st.src_off, st.src_len});
        st.src_off = L.so; L.so += ((uint64_t)st.src_len + src_slack + 15) & ~15ull;
        L.dof = (L.dof + (lz4_history && st.format == ALZ_FMT_LZ4_BLOCK ? st.aux0 : 0u) + 255) & ~255ull;
        st.dst_off = L.dof; L.dof = (L.dof + st.dst_cap + 255) & ~255ull;
        L.ds.push_back(st);
    }
    return L;
}
// ... the library's device buffers grown to the layout and its inputs uploaded
static int stage_share(alz_ctx* c, const share_layout& L) {
    int rc;
    if ((rc = grow(c, &c->d_src, &c->d_src_cap, L.so + 64))) return rc;
    if ((rc = grow(c, &c->d_dst, &c->d_dst_cap, L.dof + 64))) return rc;
    return upload_segs(c, c->d_src, L.ins, L.so);
}
// ... and the share's results (and section offsets: `ax`, an encoder's) back in the caller's tables, what the streams produced (`only_ok`: the
// streams that are ALZ_ST_OK) back in the caller's buffer
static int scatter_share(alz_ctx* c, const std::vector<uint32_t>& idx, const share_layout& L, const alz_stream* streams, const alz_result* rs, const alz_encode_aux* ax,
                         bool only_ok, uint8_t* dst_base, alz_result* results, alz_encode_aux* aux) {
    std::vector<out_seg> outs; outs.reserve(idx.size());
    for (size_t j = 0; j < idx.size(); j++) {
        results[idx[j]] = rs[j];
        if (ax && aux) aux[idx[j]] = ax[j];
        if (rs[j].dst_len && (!only_ok || rs[j].status == ALZ_ST_OK)) outs.push_back(out_seg{L.ds[j].dst_off, dst_base + streams[idx[j]].dst_off, rs[j].dst_len});
    }
    return download_segs(c, outs);
}

static int decode_share(alz_ctx* c, const alz_lz_properties* props, const std::vector<uint32_t>& idx, const uint8_t* src_base,
                        const alz_stream* streams, uint8_t* dst_base, alz_result* results) {
    const uint32_t m = (uint32_t)idx.size();
    HIP_TRY(hipSetDevice(c->device));
    const share_layout L = pack_share(idx, src_base, streams, 0, true);
    int rc;
    if ((rc = stage_share(c, L))) return rc;
    for (uint32_t j = 0; j < m; j++) {                       // LZ4 blocks that continue a frame's window: their history travels too
        const alz_stream& st = streams[idx[j]];
        if (st.format == ALZ_FMT_LZ4_BLOCK && st.aux0)
            HIP_TRY(hipMemcpyAsync((uint8_t*)c->d_dst + L.ds[j].dst_off - st.aux0, dst_base + st.dst_off - st.aux0, st.aux0, hipMemcpyHostToDevice, c->stream));
    }
    alz_plan* p = nullptr;
    if ((rc = plan_create(c, props, m, L.ds.data(), &p, true))) return rc;
    std::vector<alz_result> rs(m);
    rc = alz_plan_execute(c, p, c->d_src, c->d_dst, nullptr);
    if (!rc) rc = alz_plan_results(c, p, rs.data());
    if (rc) (void)hipStreamSynchronize(c->stream);           // (the stream table `L.ds` and the plan's index list are upload sources)
    alz_plan_destroy(c, p);
    return rc ? rc : scatter_share(c, idx, L, streams, rs.data(), nullptr, false, dst_base, results, nullptr);
}

int alz_decode_batch_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, uint32_t n,
                           const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results, uint32_t* part_of_out) {
    if (!ctxs || n_ctx == 0 || n_ctx > 64 || (n && (!streams || !results))) return fail(ALZ_E_INVALID, "alz_decode_batch_multi: bad argument");
    int rc;
    if ((rc = check_contexts("alz_decode_batch_multi", ctxs, n_ctx))) return rc;
    if ((rc = validate_streams("", ALZ_FMT_COUNT, n, streams, &src_bytes, &dst_bytes, refuse_lz4_history))) return rc;
    std::vector<uint32_t> part(n ? n : 1);
    if ((rc = alz_partition_batch(n, streams, n_ctx, part.data(), nullptr))) return rc;
    // (the shares are independent: a fresh LzWindows per stream, LZ10.cs:86)
    return run_shares(ctxs, n_ctx, n, part.data(), part_of_out, [&](uint32_t q, const std::vector<uint32_t>& idx) {
        return decode_share(ctxs[q], props, idx, src_base, streams, dst_base, results);
    });
}

// ---------------------------------------------------------------- device-resident batches over several contexts
struct alz_multi_plan {
    std::vector<alz_ctx*> ctxs;
    std::vector<alz_plan*> plans;                  // one per context (NULL: no stream of the batch went there)
    std::vector<std::vector<uint32_t>> idx;        // the batch indices of every context's streams, ascending
    uint32_t n = 0;
};
void alz_plan_destroy_multi(alz_multi_plan* mp) {
    if (!mp) return;
    for (size_t q = 0; q < mp->plans.size(); q++) if (mp->plans[q]) alz_plan_destroy(mp->ctxs[q], mp->plans[q]);
    delete mp;
}
int alz_plan_create_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, uint32_t n, const alz_stream* streams,
                          const uint32_t* part_of, alz_multi_plan** out, uint32_t* part_of_out) {
    if (!ctxs || n_ctx == 0 || n_ctx > 64 || !out || (n && !streams)) return fail(ALZ_E_INVALID, "alz_plan_create_multi: bad argument");
    if (int rc = check_contexts("alz_plan_create_multi", ctxs, n_ctx)) return rc;
    std::vector<uint32_t> part(n ? n : 1);
    if (part_of) { for (uint32_t i = 0; i < n; i++) { if (part_of[i] >= n_ctx) return fail(ALZ_E_INVALID, "alz_plan_create_multi: part_of[%u] = %u, %u contexts", i, part_of[i], n_ctx); part[i] = part_of[i]; } }
    else if (int rc = alz_partition_batch(n, streams, n_ctx, part.data(), nullptr)) return rc;
    if (part_of_out) for (uint32_t i = 0; i < n; i++) part_of_out[i] = part[i];
    alz_multi_plan* mp = new (std::nothrow) alz_multi_plan();
    if (!mp) return fail(ALZ_E_NOMEM, "out of memory");
    mp->n = n; mp->ctxs.assign(ctxs, ctxs + n_ctx); mp->plans.assign(n_ctx, nullptr); mp->idx.resize(n_ctx);
    for (uint32_t i = 0; i < n; i++) mp->idx[part[i]].push_back(i);
    std::vector<alz_stream> share;
    for (uint32_t q = 0; q < n_ctx; q++) {
        if (mp->idx[q].empty()) continue;
        share.clear();
        for (uint32_t i : mp->idx[q]) share.push_back(streams[i]);
        if (int rc = alz_plan_create(ctxs[q], props, (uint32_t)share.size(), share.data(), &mp->plans[q])) { alz_plan_destroy_multi(mp); return rc; }
    }
    *out = mp;
    return ALZ_OK;
}
int alz_plan_execute_multi(alz_multi_plan* mp, const void* const* d_src_bases, void* const* d_dst_bases) {
    if (!mp || !d_src_bases || !d_dst_bases) return fail(ALZ_E_INVALID, "alz_plan_execute_multi: bad argument");
    for (size_t q = 0; q < mp->plans.size(); q++) {
        if (!mp->plans[q]) continue;
        if (int rc = alz_plan_execute(mp->ctxs[q], mp->plans[q], d_src_bases[q], d_dst_bases[q], nullptr)) return rc;   // (asynchronous: every device works while the next is being fed)
    }
    return ALZ_OK;
}
int alz_plan_results_multi(alz_multi_plan* mp, alz_result* results) {
    if (!mp || (mp->n && !results)) return fail(ALZ_E_INVALID, "alz_plan_results_multi: bad argument");
    std::vector<alz_result> rs;
    for (size_t q = 0; q < mp->plans.size(); q++) {
        if (!mp->plans[q]) continue;
        rs.resize(mp->idx[q].size());
        if (int rc = alz_plan_results(mp->ctxs[q], mp->plans[q], rs.data())) return rc;
        for (size_t j = 0; j < rs.size(); j++) results[mp->idx[q][j]] = rs[j];
    }
    return ALZ_OK;
}

// One context's share of an encode batch: its raw buffers are packed into a device buffer of their own, the compressed streams come
// back from worst-case-sized slots.
static int encode_share(alz_ctx* c, const alz_lz_properties* props, const alz_settings* settings, const std::vector<uint32_t>& idx,
                        const uint8_t* src_base, const alz_stream* streams, uint8_t* dst_base, alz_result* results, alz_encode_aux* aux) {
    const uint32_t m = (uint32_t)idx.size();
    const share_layout L = pack_share(idx, src_base, streams, 16, false);    // (the match finder reads up to 16 bytes past a buffer: never another stream's)
    std::vector<alz_result> rs(m);
    std::vector<alz_encode_aux> ax(m);
    int rc = encode_core(c, props, settings, m, (size_t)L.so, L.ds.data(), (size_t)L.dof, rs.data(), ax.data(), [&](const void*& dsrc, void*& ddst) {
        const int r = stage_share(c, L);
        dsrc = c->d_src; ddst = c->d_dst;
        return r;
    });
    return rc ? rc : scatter_share(c, idx, L, streams, rs.data(), ax.data(), true, dst_base, results, aux);
}

// alz_encode_batch over several contexts (one per GPU): streams are independent -- a fresh LzChainMatchFinder per CompressHeaderless
// call (LZSS.cs:135) -- so the batch is dealt out by raw size (LPT) and every share runs on its own device, no collective.
int alz_encode_batch_multi(alz_ctx* const* ctxs, uint32_t n_ctx, const alz_lz_properties* props, const alz_settings* settings, uint32_t n,
                           const uint8_t* src_base, size_t src_bytes, const alz_stream* streams,
                           uint8_t* dst_base, size_t dst_bytes, alz_result* results, alz_encode_aux* aux, uint32_t* part_of_out) {
    if (!ctxs || n_ctx == 0 || n_ctx > 64 || (n && (!streams || !results || !dst_base))) return fail(ALZ_E_INVALID, "alz_encode_batch_multi: bad argument");
    int rc;
    if ((rc = check_contexts("alz_encode_batch_multi", ctxs, n_ctx))) return rc;
    if ((rc = validate_streams("", ALZ_FMT_COUNT, n, streams, &src_bytes, &dst_bytes, no_refusal))) return rc;
    // greedy LPT over the raw sizes (the cost of an encode is its positions), longest first onto the least loaded context
    std::vector<uint32_t> part(n ? n : 1);
    std::vector<uint64_t> load(n_ctx, 0);
    lpt_deal(n, n_ctx, [&](uint32_t i) { return (uint64_t)streams[i].src_len + 4096; }, part.data(), load.data());
    return run_shares(ctxs, n_ctx, n, part.data(), part_of_out, [&](uint32_t q, const std::vector<uint32_t>& idx) {
        return encode_share(ctxs[q], props, settings, idx, src_base, streams, dst_base, results, aux);
    });
}

// ---------------------------------------------------------------- measurement helper: device copy bandwidth
typedef unsigned int alz_u4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) alz_copy_kernel(const alz_u4* __restrict__ a, alz_u4* __restrict__ b, size_t n16) {
    // four 16-byte loads in flight per lane, then four stores (a block moves 16 KiB per trip)
    const size_t stride = (size_t)gridDim.x * 1024;
    size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x;
    for (; i + 768 < n16; i += stride) {
        const alz_u4 v0 = __builtin_nontemporal_load(a + i), v1 = __builtin_nontemporal_load(a + i + 256), v2 = __builtin_nontemporal_load(a + i + 512), v3 = __builtin_nontemporal_load(a + i + 768);
        __builtin_nontemporal_store(v0, b + i); __builtin_nontemporal_store(v1, b + i + 256); __builtin_nontemporal_store(v2, b + i + 512); __builtin_nontemporal_store(v3, b + i + 768);
    }
    for (; i < n16; i += 256) b[i] = a[i];
}
int alz_last_kernel_ms(alz_ctx* c, float* ms) {
    if (!c || !ms) return fail(ALZ_E_INVALID, "bad argument");
    *ms = c->last_kernel_ms;
    return ALZ_OK;
}
int alz_measure_copy_bandwidth(alz_ctx* c, size_t bytes, int iters, double* gb_per_s) {
    if (!c || !gb_per_s || iters < 1 || bytes < (1u << 20)) return fail(ALZ_E_INVALID, "alz_measure_copy_bandwidth: bad argument");
    HIP_TRY(hipSetDevice(c->device));
    void *a = nullptr, *b = nullptr;
    HIP_TRY(hipMalloc(&a, bytes));
    hipError_t e = hipMalloc(&b, bytes);
    if (e != hipSuccess) { (void)hipFree(a); return fail(ALZ_E_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e)); }
    const size_t n16 = bytes / 16;
    (void)hipMemsetAsync(a, 1, bytes, c->stream);
    alz_copy_kernel<<<dim3(256 * 8), dim3(256), 0, c->stream>>>((const alz_u4*)a, (alz_u4*)b, n16);      // warm-up
    (void)hipEventRecord(c->ev0, c->stream);
    for (int i = 0; i < iters; i++) alz_copy_kernel<<<dim3(256 * 8), dim3(256), 0, c->stream>>>((const alz_u4*)a, (alz_u4*)b, n16);
    (void)hipEventRecord(c->ev1, c->stream);
    e = hipEventSynchronize(c->ev1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev0, c->ev1);
    (void)hipFree(a); (void)hipFree(b);
    if (e != hipSuccess) return fail(ALZ_E_HIP, "copy kernel failed: %s", hipGetErrorString(e));
    *gb_per_s = 2.0 * (double)(n16 * 16) * iters / (ms * 1e-3) / 1e9;   // bytes read + bytes written
    return ALZ_OK;
}

}  // extern "C"
