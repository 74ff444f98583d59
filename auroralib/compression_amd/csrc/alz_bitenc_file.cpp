// alz_bitenc_file.cpp -- Compress of the CRILAYLA and ALLZ classes of the reference (CRI/CRILAYLA.cs:102-121, Specialized/ALLZ.cs:78-88) over
// alz_bitenc_encode_batch: one file (alz_bitenc_file_compress) and a whole set whose bodies are ONE encode batch
// (alz_bitenc_file_compress_batch).  Pure host code on the public ABI; the flow is alz_file_batch.h's, what stands here is the two classes.
#include "auroralz.h"
#include "alz_file_batch.h"

static const uint32_t kCriHeader = 0x100;                                   // HeaderSize  CRILAYLA.cs:18
static inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

namespace {
struct BitFile {
    static size_t head(const alz_stream& f) { return f.format == ALZ_BITLZ_CRILAYLA ? 16 : 12; }
    static size_t tail(const alz_stream& f) { return f.format == ALZ_BITLZ_CRILAYLA ? kCriHeader : 0; }
    static int refuse(uint32_t kind, uint32_t aux0, size_t src_len) {
        if (kind >= ALZ_BITLZ_COUNT) return ALZ_E_INVALID;
        if (kind == ALZ_BITLZ_CRILAYLA && src_len < kCriHeader) return ALZ_E_INVALID;            // "Source must be at least 256 bytes long."  :104-105
        if (kind == ALZ_BITLZ_ALLZ && ((aux0 & 0xFFu) > 24u || ((aux0 >> 8) & 0xFFu) > 24u || ((aux0 >> 16) & 0xFFu) > 24u || (aux0 >> 24))) return ALZ_E_INVALID;
        if (src_len > 0x40000000u) return ALZ_E_UNSUPPORTED;
        return ALZ_OK;
    }
    static alz_stream body(const alz_stream& f) {                               // CRILAYLA: source.Slice(HeaderSize)  :110
        alz_stream s; memset(&s, 0, sizeof(s));
        s.format = f.format; s.aux0 = f.format == ALZ_BITLZ_ALLZ ? f.aux0 : 0u;
        s.src_off = f.src_off + tail(f); s.src_len = f.src_len - (uint32_t)tail(f);
        return s;
    }
    static size_t bound(const alz_stream& s) { return alz_bitenc_bound(s.format, s.src_len); }
    static constexpr auto encode = alz_bitenc_encode_batch;
    static void frame(const alz_stream& f, const uint8_t* src, uint32_t body_len, uint8_t* d) {
        if (f.format == ALZ_BITLZ_CRILAYLA) {                                               // :111-115: the first 0x100 source bytes go behind the body
            memcpy(d, "CRILAYLA", 8); wr32(d + 8, f.src_len - kCriHeader); wr32(d + 12, body_len);
            memcpy(d + 16 + body_len, src, kCriHeader);
        } else {                                                                            // ALLZ.cs:81-84
            memcpy(d, "ALLZ", 4); d[4] = 0; d[5] = (uint8_t)f.aux0; d[6] = (uint8_t)(f.aux0 >> 8); d[7] = (uint8_t)(f.aux0 >> 16); wr32(d + 8, f.src_len);
        }
    }
};
}  // namespace

size_t alz_bitenc_file_bound(uint32_t kind, size_t src_len) {
    if (kind >= ALZ_BITLZ_COUNT || (kind == ALZ_BITLZ_CRILAYLA && src_len < kCriHeader)) return 0;
    return kind == ALZ_BITLZ_CRILAYLA ? 16 + alz_bitenc_bound(kind, src_len - kCriHeader) + kCriHeader : 12 + alz_bitenc_bound(kind, src_len);
}

int alz_bitenc_file_compress_batch(alz_ctx* ctx, const alz_settings* settings, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                   const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    return alz_file_batch::compress_bodies_batch<BitFile>(ctx, settings, n, src_base, src_bytes, files, dst_base, dst_bytes, results);
}

int alz_bitenc_file_compress(alz_ctx* ctx, uint32_t kind, const alz_settings* settings, uint32_t aux0, const uint8_t* src, size_t src_len,
                             uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    return alz_file_batch::compress_body_file<BitFile>(ctx, settings, kind, aux0, src, src_len, dst, dst_cap, dst_len);
}
