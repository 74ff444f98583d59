// alz_bitenc_file.cpp -- Compress of the CRILAYLA and ALLZ classes of the reference (CRI/CRILAYLA.cs:102-121, Specialized/ALLZ.cs:78-88) over
// alz_bitenc_encode_batch: one file (alz_bitenc_file_compress) and a whole set whose bodies are ONE encode batch
// (alz_bitenc_file_compress_batch).  Pure host code on the public ABI; the single-file call is the batch of one file.
#include <cstring>
#include <vector>

#include "auroralz.h"

static const uint32_t kCriHeader = 0x100;                                   // HeaderSize  CRILAYLA.cs:18
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
static inline size_t head_bytes(uint32_t kind) { return kind == ALZ_BITLZ_CRILAYLA ? 16 : 12; }
static inline size_t tail_bytes(uint32_t kind) { return kind == ALZ_BITLZ_CRILAYLA ? kCriHeader : 0; }
static inline size_t body_src(uint32_t kind, size_t src_len) { return kind == ALZ_BITLZ_CRILAYLA ? src_len - kCriHeader : src_len; }   // source.Slice(HeaderSize)  :110

size_t alz_bitenc_file_bound(uint32_t kind, size_t src_len) {
    if (kind >= ALZ_BITLZ_COUNT || (kind == ALZ_BITLZ_CRILAYLA && src_len < kCriHeader)) return 0;
    return head_bytes(kind) + alz_bitenc_bound(kind, body_src(kind, src_len)) + tail_bytes(kind);
}

// what the single-file call refuses before anything runs
static int refuse_file(uint32_t kind, uint32_t aux0, size_t src_len) {
    if (kind >= ALZ_BITLZ_COUNT) return ALZ_E_INVALID;
    if (kind == ALZ_BITLZ_CRILAYLA && src_len < kCriHeader) return ALZ_E_INVALID;            // "Source must be at least 256 bytes long."  :104-105
    if (kind == ALZ_BITLZ_ALLZ && ((aux0 & 0xFFu) > 24u || ((aux0 >> 8) & 0xFFu) > 24u || ((aux0 >> 16) & 0xFFu) > 24u || (aux0 >> 24))) return ALZ_E_INVALID;
    if (src_len > 0x40000000u) return ALZ_E_UNSUPPORTED;
    return ALZ_OK;
}

int alz_bitenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                   const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (!ctx || (n && (!files || !results || !dst_base)) || (src_bytes && !src_base)) return ALZ_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (files[i].src_off > src_bytes || files[i].src_len > src_bytes - files[i].src_off) return ALZ_E_INVALID;
        if (files[i].dst_off > dst_bytes || files[i].dst_cap > dst_bytes - files[i].dst_off) return ALZ_E_INVALID;
    }
    if (n == 0) return ALZ_OK;
    // the bodies of the files that pass their own checks: one stream each, sources where they lie, a slot of the body's bound each
    std::vector<alz_stream> st; std::vector<uint32_t> file_of; size_t slots = 0;
    for (uint32_t i = 0; i < n; i++) {
        const alz_stream& f = files[i];
        alz_file_result& r = results[i]; r.rc = refuse_file(f.format, f.aux0, f.src_len); r.status = ALZ_ST_OK; r.dst_len = 0; r.src_used = 0;
        if (r.rc) continue;
        alz_stream s; memset(&s, 0, sizeof(s));
        const size_t bs = body_src(f.format, f.src_len), bound = alz_bitenc_bound(f.format, bs);
        if (bound > 0xFFFFFFFFull) { r.rc = ALZ_E_UNSUPPORTED; continue; }
        s.format = f.format; s.aux0 = f.format == ALZ_BITLZ_ALLZ ? f.aux0 : 0u;
        s.src_off = f.src_off + (f.src_len - bs); s.src_len = (uint32_t)bs;
        s.dst_off = slots; s.dst_cap = (uint32_t)bound;
        slots += (bound + 63) & ~(size_t)63;
        st.push_back(s); file_of.push_back(i);
    }
    if (st.empty()) return ALZ_OK;
    std::vector<uint8_t> bodies(slots + 64);
    std::vector<alz_result> br(st.size());
    if (const int rc = alz_bitenc_encode_batch(ctx, settings, (uint32_t)st.size(), src_base, src_bytes, st.data(), bodies.data(), slots, br.data())) return rc;
    for (size_t k = 0; k < st.size(); k++) {
        const alz_stream& f = files[file_of[k]]; alz_file_result& r = results[file_of[k]];
        if (br[k].status != ALZ_ST_OK) { r.rc = ALZ_E_STREAM; r.status = br[k].status; continue; }   // (the bound holds: not reached)
        const size_t h = head_bytes(f.format), t = tail_bytes(f.format), total = h + br[k].dst_len + t;
        if (total > f.dst_cap) { r.rc = ALZ_E_NOMEM; continue; }
        uint8_t* d = dst_base + f.dst_off; const uint8_t* src = src_base + f.src_off;
        if (f.format == ALZ_BITLZ_CRILAYLA) {                                               // :111-115
            memcpy(d, "CRILAYLA", 8); wr32(d + 8, f.src_len - kCriHeader); wr32(d + 12, br[k].dst_len);
        } else {                                                                            // ALLZ.cs:81-84
            memcpy(d, "ALLZ", 4); d[4] = 0; d[5] = (uint8_t)f.aux0; d[6] = (uint8_t)(f.aux0 >> 8); d[7] = (uint8_t)(f.aux0 >> 16); wr32(d + 8, f.src_len);
        }
        if (br[k].dst_len) memcpy(d + h, bodies.data() + st[k].dst_off, br[k].dst_len);
        if (t) memcpy(d + h + br[k].dst_len, src, t);
        r.dst_len = (uint32_t)total; r.src_used = f.src_len;
    }
    return ALZ_OK;
}

int alz_bitenc_file_compress(alz_ctx* ctx, uint32_t kind, const alz_settings* settings, uint32_t aux0, const uint8_t* src, size_t src_len,
                             uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    if (dst_len) *dst_len = 0;
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (const int rc = refuse_file(kind, aux0, src_len)) return rc;
    if (!dst) return ALZ_E_NOMEM;
    alz_stream f; memset(&f, 0, sizeof(f));
    f.format = kind; f.aux0 = aux0; f.src_len = (uint32_t)src_len; f.dst_cap = dst_cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dst_cap;
    alz_file_result r; memset(&r, 0, sizeof(r));
    if (const int rc = alz_bitenc_file_compress_batch(ctx, settings, 1, src, src_len, &f, dst, f.dst_cap, &r)) return rc;
    if (r.rc) return r.rc;
    if (dst_len) *dst_len = r.dst_len;
    return ALZ_OK;
}
