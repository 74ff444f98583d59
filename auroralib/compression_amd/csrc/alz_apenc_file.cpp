// alz_apenc_file.cpp -- Compress of the aPLib class of the reference (Formats/Common/aPLib.cs:87-103) over alz_apenc_encode_batch: one file
// (alz_apenc_file_compress) and a whole set whose bodies are ONE encode batch (alz_apenc_file_compress_batch).  Pure host code on the public
// ABI; the single-file call is the batch of one file.
#include <cstring>
#include <vector>

#include "auroralz.h"

static const size_t kHeader = 24;                                             // 'AP32', header size, compressed size, CRC, original size, CRC  :94-99
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

size_t alz_apenc_file_bound(size_t src_len) { return kHeader + alz_apenc_bound(src_len); }

// what the single-file call refuses before anything runs
static int refuse_file(size_t src_len) {
    if (src_len == 0) return ALZ_E_INVALID;                                   // source[srcPtr++] of an empty span throws  :191
    if (src_len > 0x40000000u) return ALZ_E_UNSUPPORTED;
    return ALZ_OK;
}

int alz_apenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
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
        alz_file_result& r = results[i]; r.rc = refuse_file(f.src_len); r.status = ALZ_ST_OK; r.dst_len = 0; r.src_used = 0;
        if (r.rc) continue;
        alz_stream s; memset(&s, 0, sizeof(s));
        const size_t bound = alz_apenc_bound(f.src_len);
        s.src_off = f.src_off; s.src_len = f.src_len;
        s.dst_off = slots; s.dst_cap = (uint32_t)bound;
        slots += (bound + 63) & ~(size_t)63;
        st.push_back(s); file_of.push_back(i);
    }
    if (st.empty()) return ALZ_OK;
    std::vector<uint8_t> bodies(slots + 64);
    std::vector<alz_result> br(st.size());
    if (const int rc = alz_apenc_encode_batch(ctx, settings, (uint32_t)st.size(), src_base, src_bytes, st.data(), bodies.data(), slots, br.data())) return rc;
    for (size_t k = 0; k < st.size(); k++) {
        const alz_stream& f = files[file_of[k]]; alz_file_result& r = results[file_of[k]];
        if (br[k].status != ALZ_ST_OK) { r.rc = ALZ_E_STREAM; r.status = br[k].status; continue; }   // (the bound holds: not reached)
        const size_t total = kHeader + br[k].dst_len;
        if (total > f.dst_cap) { r.rc = ALZ_E_NOMEM; continue; }
        uint8_t* d = dst_base + f.dst_off;
        memcpy(d, "AP32", 4); wr32(d + 4, (uint32_t)kHeader); wr32(d + 8, br[k].dst_len); wr32(d + 12, 0); wr32(d + 16, f.src_len); wr32(d + 20, 0);
        memcpy(d + kHeader, bodies.data() + st[k].dst_off, br[k].dst_len);
        r.dst_len = (uint32_t)total; r.src_used = f.src_len;
    }
    return ALZ_OK;
}

int alz_apenc_file_compress(alz_ctx* ctx, const alz_settings* settings, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    if (dst_len) *dst_len = 0;
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (const int rc = refuse_file(src_len)) return rc;
    if (!dst) return ALZ_E_NOMEM;
    alz_stream f; memset(&f, 0, sizeof(f));
    f.src_len = (uint32_t)src_len; f.dst_cap = dst_cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dst_cap;
    alz_file_result r; memset(&r, 0, sizeof(r));
    if (const int rc = alz_apenc_file_compress_batch(ctx, settings, 1, src, src_len, &f, dst, f.dst_cap, &r)) return rc;
    if (r.rc) return r.rc;
    if (dst_len) *dst_len = r.dst_len;
    return ALZ_OK;
}
