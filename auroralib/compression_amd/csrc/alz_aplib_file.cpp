// alz_aplib_file.cpp -- the aPLib class of the reference (Formats/Common/aPLib.cs:39-84) over alz_aplib_decode_batch: IsMatch,
// GetDecompressedSize and Decompress(Stream, Stream) of an "AP32" file or a headerless body.  Pure host code on the public ABI.
#include <cstring>

#include "auroralz.h"

static inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline bool has_magic(const uint8_t* src, size_t len) { return src && len >= 4 && memcmp(src, "AP32", 4) == 0; }

// IsMatchStatic  aPLib.cs:43-44: Position + 0x10 < Length && Match("AP32") && ReadUInt32() == 24
int alz_aplib_is_match(const uint8_t* src, size_t src_len) {
    return src_len > 0x10 && has_magic(src, src_len) && rd32(src + 4) == 24u;
}

// GetDecompressedSize  aPLib.cs:47-53: MatchThrow, skip 12, ReadUInt32
int alz_aplib_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out) {
    if (!size_out) return ALZ_E_INVALID;
    if (!has_magic(src, src_len) || src_len < 20) return ALZ_E_FORMAT;
    *size_out = rd32(src + 16);
    return ALZ_OK;
}

// Decompress  aPLib.cs:56-84
int alz_aplib_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                         size_t* dst_len, size_t* src_used, int32_t* status) {
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (dst_len) *dst_len = 0;
    if (src_used) *src_used = 0;
    if (status) *status = ALZ_ST_OK;
    const bool file = has_magic(src, src_len);                              // no magic (or fewer than 4 bytes): a headerless body  :59-64
    uint64_t start = 0; uint32_t want = 0;
    if (file) {
        if (src_len < 24) return ALZ_E_FORMAT;                              // the six header words are read unconditionally  :65-69
        want = rd32(src + 16);
        start = 24ull + (uint32_t)(rd32(src + 4) - 24u);                    // source.Position += (uint)(headerSize - 24)  :70
    }
    if (start > src_len) {                                                  // Position beyond the end: the first ReadUInt8 throws
        if (status) *status = ALZ_ST_INPUT_TRUNCATED;
        if (src_used) *src_used = src_len;
        return ALZ_E_STREAM;
    }
    const uint64_t body = src_len - start;
    if (body > 0xFFFFFFFFull) return ALZ_E_UNSUPPORTED;                     // alz_stream counts in 32 bits
    alz_stream st; memset(&st, 0, sizeof(st));
    st.src_len = (uint32_t)body;
    st.dst_cap = dst_cap > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)dst_cap;
    alz_result r; memset(&r, 0, sizeof(r));
    const int rc = alz_aplib_decode_batch(ctx, 1, src + start, (size_t)body, &st, dst, st.dst_cap, &r);
    if (rc) return rc;
    if (dst_len) *dst_len = r.dst_len;
    if (src_used) *src_used = (size_t)start + r.src_used;
    int stt = r.status;
    if (stt == ALZ_ST_OK && file && r.dst_len != want) stt = ALZ_ST_OUTPUT_SIZE_MISMATCH;   // DecompressedSizeException  :81-83 (a compressed-size mismatch is only traced, :78)
    if (status) *status = stt;
    return stt == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}
