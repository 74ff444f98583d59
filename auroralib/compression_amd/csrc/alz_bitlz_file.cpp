// alz_bitlz_file.cpp -- the CRILAYLA and ALLZ classes of the reference (CRI/CRILAYLA.cs:34-99, Specialized/ALLZ.cs:39-75) over
// alz_bitlz_decode_batch: IsMatch, GetDecompressedSize and Decompress(Stream, Stream) of a whole file.  Pure host code on the public ABI.
#include <cstring>

#include "auroralz.h"

static inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline bool has_magic(const uint8_t* src, size_t len, const char* magic, size_t n) { return src && len >= n && memcmp(src, magic, n) == 0; }
static const uint32_t kCriHeader = 0x100;                                   // HeaderSize  CRILAYLA.cs:18

// ---------------------------------------------------------------------------------------------- CRILAYLA
// IsMatchStatic  CRILAYLA.cs:34-35: Length > 0x10 && Match("CRILAYLA")
int alz_crilayla_is_match(const uint8_t* src, size_t src_len) {
    return src_len > 0x10 && has_magic(src, src_len, "CRILAYLA", 8);
}

// GetDecompressedSize  CRILAYLA.cs:58-63: MatchThrow, ReadUInt32() + 0x100 (a uint sum)
int alz_crilayla_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out) {
    if (!size_out) return ALZ_E_INVALID;
    if (!has_magic(src, src_len, "CRILAYLA", 8) || src_len < 12) return ALZ_E_FORMAT;
    *size_out = rd32(src + 8) + kCriHeader;
    return ALZ_OK;
}

// Decompress  CRILAYLA.cs:66-99
int alz_crilayla_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                            size_t* dst_len, size_t* src_used, int32_t* status) {
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (dst_len) *dst_len = 0;
    if (src_used) *src_used = 0;
    if (status) *status = ALZ_ST_OK;
    if (src_len < 16 || !has_magic(src, src_len, "CRILAYLA", 8)) return ALZ_E_FORMAT;
    const uint32_t size = rd32(src + 8), csize = rd32(src + 12);
    const uint64_t full = (uint64_t)size + kCriHeader;
    if (full >= 0x80000000ull) return ALZ_E_UNSUPPORTED;                    // int fullSize = (int)(decompressedSize + HeaderSize)  :72
    if (16ull + csize > src_len) {                                          // source.Read comes back short: the body's last bytes are missing
        if (status) *status = ALZ_ST_INPUT_TRUNCATED;
        if (src_used) *src_used = src_len;
        return ALZ_E_STREAM;
    }
    if (dst_cap < full) {
        if (status) *status = ALZ_ST_OUTPUT_CAPACITY;
        return ALZ_E_STREAM;
    }
    const size_t left = src_len - 16 - csize, hdr = left < kCriHeader ? left : (size_t)kCriHeader;
    memset(dst, 0, (size_t)full);                                           // what neither the header nor the body writes
    memcpy(dst, src + 16 + csize, hdr);                                     // source.Read(destinationBuffer, 0, HeaderSize)  :79
    alz_stream st; memset(&st, 0, sizeof(st));
    st.src_len = csize; st.dst_cap = (uint32_t)full; st.format = ALZ_BITLZ_CRILAYLA;
    alz_result r; memset(&r, 0, sizeof(r));
    // the body is decoded over the top of the span and may reach into the header region (:81): only what it produced is copied back
    const int rc = alz_bitlz_decode_batch(ctx, 1, src + 16, csize, &st, dst, (size_t)full, &r);
    if (rc) return rc;
    if (src_used) *src_used = 16 + (size_t)csize + hdr;
    int stt = r.status;
    if (stt == ALZ_ST_OK && r.dst_len < size) stt = ALZ_ST_OUTPUT_SIZE_MISMATCH;   // DecompressedSizeException, thrown behind destination.Write  :86-92
    if (status) *status = stt;
    if (dst_len && (stt == ALZ_ST_OK || stt == ALZ_ST_OUTPUT_SIZE_MISMATCH)) *dst_len = (size_t)full;   // (a body error delivers nothing)
    return stt == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}

// ---------------------------------------------------------------------------------------------- ALLZ
// IsMatchStatic  ALLZ.cs:43-44: Position + 0x10 < Length && Match("ALLZ")
int alz_allz_is_match(const uint8_t* src, size_t src_len) {
    return src_len > 0x10 && has_magic(src, src_len, "ALLZ", 4);
}

// GetDecompressedSize  ALLZ.cs:47-53: MatchThrow, skip 4, ReadUInt32
int alz_allz_decompressed_size(const uint8_t* src, size_t src_len, uint32_t* size_out) {
    if (!size_out) return ALZ_E_INVALID;
    if (!has_magic(src, src_len, "ALLZ", 4) || src_len < 12) return ALZ_E_FORMAT;
    *size_out = rd32(src + 8);
    return ALZ_OK;
}

// Decompress  ALLZ.cs:56-75
int alz_allz_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status) {
    if (!ctx || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    if (dst_len) *dst_len = 0;
    if (src_used) *src_used = 0;
    if (status) *status = ALZ_ST_OK;
    if (src_len < 12 || !has_magic(src, src_len, "ALLZ", 4)) return ALZ_E_FORMAT;
    const uint32_t size = rd32(src + 8);
    if (size >= 0x80000000u) return ALZ_E_UNSUPPORTED;                      // Rent((int)decompressedSize)  :65
    const uint64_t body = src_len - 12;
    if (body > 0xFFFFFFFFull) return ALZ_E_UNSUPPORTED;                     // alz_stream counts in 32 bits
    alz_stream st; memset(&st, 0, sizeof(st));
    st.src_len = (uint32_t)body;
    st.dst_cap = dst_cap < size ? (uint32_t)dst_cap : size;                 // (nothing beyond `size` is ever written: the staging buffer need not hold the caller's whole capacity)
    st.decom_len = size;
    st.aux0 = ALZ_ALLZ_AUX0((uint32_t)src[5], (uint32_t)src[6], (uint32_t)src[7]);   // flags[1..3]  :60-61
    st.format = ALZ_BITLZ_ALLZ;
    alz_result r; memset(&r, 0, sizeof(r));
    const int rc = alz_bitlz_decode_batch(ctx, 1, src + 12, (size_t)body, &st, dst, st.dst_cap, &r);
    if (rc) return rc;
    if (dst_len) *dst_len = r.dst_len;
    if (src_used) *src_used = 12 + (size_t)r.src_used;
    if (status) *status = r.status;
    return r.status == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}
