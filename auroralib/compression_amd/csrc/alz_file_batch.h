// alz_file_batch.h -- what the file layers share.  The batched ones (alz_zfile.cpp: ZLib / GZip; alz_framed_batch.cpp and
// alz_framing_compress.cpp: LZ4 / Snappy): their argument check and the one download of all outputs.  Those and the single-file layer
// (alz_container.cpp): a device buffer that is freed on every exit path, the plan runner, and the split of a set of streams into long
// blocks and short ones.  The writers of the bit-stream file classes (alz_bitenc_file.cpp, alz_apenc_file.cpp): their whole flow, over the
// class's own refusals, body and frame.  Pure host code on the public ABI; not part of it.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "auroralz.h"

namespace alz_file_batch {

struct DeviceBuffer {                                                           // freed on every exit path
    alz_ctx* ctx; void* p = nullptr;
    explicit DeviceBuffer(alz_ctx* c) : ctx(c) {}
    ~DeviceBuffer() { if (p) (void)alz_device_free(ctx, p); }
    int alloc(size_t bytes) { return alz_device_malloc(ctx, bytes ? bytes : 1, &p); }
};

inline bool range_ok(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }

// the argument check of a batched file call: accepts(format) names the files it reads; has_dst: the call writes outputs
template <class Accepts>
inline int check_files(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, const uint8_t* dst_base, size_t dst_bytes,
                       const alz_file_result* results, bool has_dst, Accepts accepts) {
    if (!ctx || (n && (!files || !results)) || (src_bytes && !src_base) || (has_dst && dst_bytes && !dst_base)) return ALZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (!accepts(files[i].format)) return ALZ_E_INVALID;
        if (!range_ok(files[i].src_off, files[i].src_len, src_bytes)) return ALZ_E_INVALID;
        if (has_dst && !range_ok(files[i].dst_off, files[i].dst_cap, dst_bytes)) return ALZ_E_INVALID;
    }
    return ALZ_OK;
}

// runs the streams `ss` as one plan, device-resident, and returns their results
inline int run_plan(alz_ctx* ctx, std::vector<alz_stream>& ss, std::vector<alz_result>& rs, const void* d_src, void* d_dst) {
    alz_plan* pl = nullptr; rs.resize(ss.size());
    int e = alz_plan_create(ctx, nullptr, (uint32_t)ss.size(), ss.data(), &pl);
    if (e != ALZ_OK) return e;
    e = alz_plan_execute(ctx, pl, d_src, d_dst, nullptr);
    if (e == ALZ_OK) e = alz_plan_results(ctx, pl, rs.data());
    alz_plan_destroy(ctx, pl);
    return e;
}
// (worth the whole GPU by itself: plan_create's own test, restated for the split below -- a wrong guess costs time, not bytes)
inline bool long_block(const alz_stream& s) { return s.format == ALZ_FMT_LZ4_BLOCK && s.src_len >= 8192u && s.dst_cap >= (24u << 10); }
// A plan takes its streams one after the other on the whole GPU only when ALL of them are worth it (plan_create), and the last block of a
// file is usually a short one: 16 MB in 4 MiB blocks -- four of them and 2 KB -- decoded every block on wavefronts of its own, 14 ms for
// the 4 MiB ones instead of 0.5 each.  So the long blocks and the short ones go out as two plans, unless there are more than 32 long ones;
// `rs` in the order of `ss`, *split: whether two plans ran.
inline int run_long_and_short(alz_ctx* ctx, std::vector<alz_stream>& ss, std::vector<alz_result>& rs, const void* d_src, void* d_dst, bool* split) {
    std::vector<alz_stream> sa, sb; std::vector<size_t> ia, ib;
    for (size_t k = 0; k < ss.size(); k++) { if (long_block(ss[k])) { sa.push_back(ss[k]); ia.push_back(k); } else { sb.push_back(ss[k]); ib.push_back(k); } }
    *split = !sa.empty() && !sb.empty() && sa.size() <= 32;
    rs.resize(ss.size());
    if (!*split) return ss.empty() ? ALZ_OK : run_plan(ctx, ss, rs, d_src, d_dst);
    std::vector<alz_result> ra, rb;
    if (int e = run_plan(ctx, sa, ra, d_src, d_dst)) return e;
    if (int e = run_plan(ctx, sb, rb, d_src, d_dst)) return e;
    for (size_t k = 0; k < ia.size(); k++) rs[ia[k]] = ra[k];
    for (size_t k = 0; k < ib.size(); k++) rs[ib[k]] = rb[k];
    return ALZ_OK;
}

// the produced bytes of every file, device -> host: neighbouring outputs travel as one copy (through a bounce buffer, so that nothing
// between two outputs is written on the host)
inline int download(alz_ctx* ctx, uint32_t n, const alz_stream* files, const alz_file_result* results, const void* d_dst, uint8_t* dst) {
    const size_t kGap = 64u << 10, kPiece = 64u << 20;
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; i++) if (results[i].dst_len) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return files[a].dst_off < files[b].dst_off; });
    std::vector<uint8_t> bounce;
    for (size_t k = 0; k < order.size();) {
        const uint64_t lo = files[order[k]].dst_off;
        uint64_t hi = lo + results[order[k]].dst_len;
        size_t e = k + 1;
        for (; e < order.size(); e++) {
            const uint64_t a = files[order[e]].dst_off, b = a + results[order[e]].dst_len;
            if (a > hi + kGap || (b > hi ? b : hi) - lo > kPiece) break;
            if (b > hi) hi = b;
        }
        if (e == k + 1) {                                                       // a lone output goes straight to its place
            if (int rc = alz_memcpy_d2h(ctx, dst + lo, (const uint8_t*)d_dst + lo, (size_t)(hi - lo))) return rc;
        } else {
            bounce.resize((size_t)(hi - lo));
            if (int rc = alz_memcpy_d2h(ctx, bounce.data(), (const uint8_t*)d_dst + lo, bounce.size())) return rc;
            for (size_t j = k; j < e; j++)
                memcpy(dst + files[order[j]].dst_off, bounce.data() + (files[order[j]].dst_off - lo), results[order[j]].dst_len);
        }
        k = e;
    }
    return ALZ_OK;
}

// Compress of a file class that is a frame around ONE encoded body (CRILAYLA, ALLZ, AP32): the files' bodies are one encode batch into host
// slots of their bounds, then every file gets its frame and its body.  What a class C says:
//   int    C::refuse(format, aux0, src_len)   what is refused of one file before anything runs (ALZ_OK: nothing)
//   alz_stream C::body(f)                     the body's stream: format, aux0 and the slice of f's source (src_off, src_len), zero elsewhere
//   size_t C::bound(s)                        the encoder's bound for that stream
//   int    C::encode(ctx, settings, n, src_base, src_bytes, streams, dst_base, dst_bytes, results)
//   size_t C::head(f), C::tail(f)             the bytes in front of the body and behind it
//   void   C::frame(f, src, body_len, d)      writes both around a body of body_len bytes at d + head(f); src: the file's source
template <class C>
inline int compress_bodies_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                                 uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (!ctx || (n && (!files || !results || !dst_base)) || (src_bytes && !src_base)) return ALZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++)
        if (!range_ok(files[i].src_off, files[i].src_len, src_bytes) || !range_ok(files[i].dst_off, files[i].dst_cap, dst_bytes)) return ALZ_E_INVALID;
    if (n == 0) return ALZ_OK;
    // the bodies of the files that pass their own checks: one stream each, sources where they lie, a slot of the body's bound each
    std::vector<alz_stream> st; std::vector<uint32_t> file_of; size_t slots = 0;
    for (uint32_t i = 0; i < n; i++) {
        const alz_stream& f = files[i];
        alz_file_result& r = results[i]; r.rc = C::refuse(f.format, f.aux0, f.src_len); r.status = ALZ_ST_OK; r.dst_len = 0; r.src_used = 0;
        if (r.rc) continue;
        alz_stream s = C::body(f);
        const size_t bound = C::bound(s);
        if (bound > 0xFFFFFFFFull) { r.rc = ALZ_E_UNSUPPORTED; continue; }
        s.dst_off = slots; s.dst_cap = (uint32_t)bound;
        slots += (bound + 63) & ~(size_t)63;
        st.push_back(s); file_of.push_back(i);
    }
    if (st.empty()) return ALZ_OK;
    std::vector<uint8_t> bodies(slots + 64);
    std::vector<alz_result> br(st.size());
    if (const int rc = C::encode(ctx, settings, (uint32_t)st.size(), src_base, src_bytes, st.data(), bodies.data(), slots, br.data())) return rc;
    for (size_t k = 0; k < st.size(); k++) {
        const alz_stream& f = files[file_of[k]]; alz_file_result& r = results[file_of[k]];
        if (br[k].status != ALZ_ST_OK) { r.rc = ALZ_E_STREAM; r.status = br[k].status; continue; }   // (the bound holds: not reached)
        const size_t h = C::head(f), total = h + br[k].dst_len + C::tail(f);
        if (total > f.dst_cap) { r.rc = ALZ_E_NOMEM; continue; }
        uint8_t* d = dst_base + f.dst_off;
        C::frame(f, src_base + f.src_off, br[k].dst_len, d);
        if (br[k].dst_len) memcpy(d + h, bodies.data() + st[k].dst_off, br[k].dst_len);
        r.dst_len = (uint32_t)total; r.src_used = f.src_len;
    }
    return ALZ_OK;
}
// ... and of one file: the batch of one
template <class C>
inline int compress_body_file(alz_ctx* ctx, const alz_settings* settings, uint32_t format, uint32_t aux0, const uint8_t* src, size_t src_len,
                              uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    if (dst_len) *dst_len = 0;
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (const int rc = C::refuse(format, aux0, src_len)) return rc;
    if (!dst) return ALZ_E_NOMEM;
    alz_stream f; memset(&f, 0, sizeof(f));
    f.format = format; f.aux0 = aux0; f.src_len = (uint32_t)src_len; f.dst_cap = dst_cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dst_cap;
    alz_file_result r; memset(&r, 0, sizeof(r));
    if (const int rc = compress_bodies_batch<C>(ctx, settings, 1, src, src_len, &f, dst, f.dst_cap, &r)) return rc;
    if (r.rc) return r.rc;
    if (dst_len) *dst_len = r.dst_len;
    return ALZ_OK;
}

}   // namespace alz_file_batch
