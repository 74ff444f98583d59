// alz_apenc_file.cpp -- Compress of the aPLib class of the reference (Formats/Common/aPLib.cs:87-103) over alz_apenc_encode_batch: one file
// (alz_apenc_file_compress) and a whole set whose bodies are ONE encode batch (alz_apenc_file_compress_batch).  Pure host code on the public
// ABI; the flow is alz_file_batch.h's, what stands here is the class.
#include "auroralz.h"
#include "alz_file_batch.h"

static const size_t kHeader = 24;                                             // 'AP32', header size, compressed size, CRC, original size, CRC  :94-99
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

namespace {
struct Ap32File {
    static size_t head(const alz_stream&) { return kHeader; }
    static size_t tail(const alz_stream&) { return 0; }
    static int refuse(uint32_t, uint32_t, size_t src_len) {
        if (src_len == 0) return ALZ_E_INVALID;                               // source[srcPtr++] of an empty span throws  :191
        if (src_len > 0x40000000u) return ALZ_E_UNSUPPORTED;
        return ALZ_OK;
    }
    static alz_stream body(const alz_stream& f) {                             // the whole source; the stream's format and aux0 are not read
        alz_stream s; memset(&s, 0, sizeof(s));
        s.src_off = f.src_off; s.src_len = f.src_len;
        return s;
    }
    static size_t bound(const alz_stream& s) { return alz_apenc_bound(s.src_len); }
    static constexpr auto encode = alz_apenc_encode_batch;
    static void frame(const alz_stream& f, const uint8_t*, uint32_t body_len, uint8_t* d) {
        memcpy(d, "AP32", 4); wr32(d + 4, (uint32_t)kHeader); wr32(d + 8, body_len); wr32(d + 12, 0); wr32(d + 16, f.src_len); wr32(d + 20, 0);
    }
};
}  // namespace

size_t alz_apenc_file_bound(size_t src_len) { return kHeader + alz_apenc_bound(src_len); }

int alz_apenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                  const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    return alz_file_batch::compress_bodies_batch<Ap32File>(ctx, settings, n, src_base, src_bytes, files, dst_base, dst_bytes, results);
}

int alz_apenc_file_compress(alz_ctx* ctx, const alz_settings* settings, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    return alz_file_batch::compress_body_file<Ap32File>(ctx, settings, 0u, 0u, src, src_len, dst, dst_cap, dst_len);
}
