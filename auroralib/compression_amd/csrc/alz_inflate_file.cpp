// alz_inflate_file.cpp -- the ZLib and GZip classes of the reference (Formats/Common/ZLib.cs, GZip.cs) over alz_inflate_decode_batch /
// alz_inflate_measure_batch: IsMatch, Decompress(Stream, Stream) and the size of a file without decoding it.  The reference hands both
// bodies to the BCL, so the framing is RFC 1950 (zlib) and RFC 1952 (gzip) as zlib reads them; checksums are computed here, on the host,
// over the downloaded output.  Pure host code on the public ABI.
#include <cstring>

#include "auroralz.h"

namespace {

const uint32_t kMaxCap = 0xFFFFFF00u;                                          // the largest dst_cap of a stream

uint32_t adler32(const uint8_t* p, size_t n) {
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = n < 5552 ? n : 5552;                                         // the longest run whose sums stay below 2^32
        n -= k;
        while (k--) { a += *p++; b += a; }
        a %= 65521u; b %= 65521u;
    }
    return (b << 16) | a;
}

struct Crc32 {
    uint32_t t[256];
    Crc32() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
    uint32_t of(const uint8_t* p, size_t n) const {
        uint32_t c = 0xFFFFFFFFu;
        while (n--) c = t[(c ^ *p++) & 0xFFu] ^ (c >> 8);
        return ~c;
    }
};
const Crc32 kCrc;

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[3] | ((uint32_t)p[2] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[0] << 24); }

// what one call reports; `out` counts the bytes delivered (decode) or counted (measure)
struct Outcome {
    size_t* dst_len; size_t* src_used; int32_t* status; bool measure;
    int end(int rc, int32_t st, size_t out, size_t used) const {
        if (dst_len) *dst_len = out;
        if (src_used) *src_used = used;
        if (status) *status = st;
        return rc;
    }
    int stream(int32_t st, size_t out, size_t used) const { return end(ALZ_E_STREAM, st, out, used); }
};

// one raw DEFLATE body at src[pos..len) into dst + out (measure: counted against `cap` only); the result in r.  The header walks in front of
// it need no context: a missing one is refused here.
int body(alz_ctx* ctx, const uint8_t* src, size_t len, size_t pos, uint8_t* dst, size_t cap, size_t out, bool measure, alz_result* r) {
    if (!ctx) return ALZ_E_INVALID;
    const size_t n = len - pos, room = cap - out;
    if (n > 0xFFFFFFFFull) return ALZ_E_UNSUPPORTED;                            // alz_stream counts in 32 bits
    alz_stream st; memset(&st, 0, sizeof(st));
    st.src_len = (uint32_t)n;
    st.dst_cap = room > kMaxCap ? kMaxCap : (uint32_t)room;
    memset(r, 0, sizeof(*r));
    return measure ? alz_inflate_measure_batch(ctx, 1, src + pos, n, &st, r)
                   : alz_inflate_decode_batch(ctx, 1, src + pos, n, &st, dst ? dst + out : nullptr, st.dst_cap, r);
}

// RFC 1950: CMF, FLG, the body, the big-endian Adler-32 of the output
int zlib_file(alz_ctx* ctx, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, const Outcome& o) {
    if (len < 2) return ALZ_E_FORMAT;
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf & 0x0Fu) != 8u) return ALZ_E_FORMAT;                               // CM
    if ((cmf >> 4) > 7u) return ALZ_E_FORMAT;                                   // CINFO (it does not limit distances: inflate with 15 window bits)
    if ((cmf * 256u + flg) % 31u != 0u) return ALZ_E_FORMAT;                    // FCHECK
    if (flg & 0x20u) return ALZ_E_UNSUPPORTED;                                  // FDICT: no preset dictionaries
    alz_result r;
    if (int rc = body(ctx, src, len, 2, dst, cap, 0, o.measure, &r)) return rc;
    if (r.status != ALZ_ST_OK) return o.stream(r.status, r.dst_len, 2 + (size_t)r.src_used);
    const size_t pos = 2 + (size_t)r.src_used;
    if (len - pos < 4) return o.stream(ALZ_ST_INPUT_TRUNCATED, r.dst_len, len);
    if (!o.measure && be32(src + pos) != adler32(dst, r.dst_len)) return o.end(ALZ_E_CHECKSUM, ALZ_ST_OK, r.dst_len, pos + 4);
    return o.end(ALZ_OK, ALZ_ST_OK, r.dst_len, pos + 4);
}

// the header of one gzip member at src[pos..len): ALZ_OK and pos behind it, ALZ_E_FORMAT, ALZ_E_CHECKSUM, or ALZ_E_STREAM (it runs past the input)
int gzip_header(const uint8_t* src, size_t len, size_t& pos) {
    const size_t start = pos, n = len - pos;
    if (n < 2 || src[pos] != 0x1F || src[pos + 1] != 0x8B) return ALZ_E_FORMAT;
    if (n >= 3 && src[pos + 2] != 8) return ALZ_E_FORMAT;                       // CM
    if (n >= 4 && (src[pos + 3] & 0xE0u)) return ALZ_E_FORMAT;                  // reserved FLG bits
    if (n < 10) return ALZ_E_STREAM;
    const uint32_t flg = src[pos + 3];
    pos += 10;                                                                  // MTIME, XFL, OS are not looked at
    if (flg & 4u) {                                                             // FEXTRA: XLEN, then XLEN bytes
        if (len - pos < 2) return ALZ_E_STREAM;
        const size_t xlen = (size_t)src[pos] | ((size_t)src[pos + 1] << 8);
        pos += 2;
        if (len - pos < xlen) return ALZ_E_STREAM;
        pos += xlen;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {                            // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        const void* z = memchr(src + pos, 0, len - pos);
        if (!z) return ALZ_E_STREAM;
        pos = (size_t)((const uint8_t*)z - src) + 1;
    }
    if (flg & 2u) {                                                             // FHCRC: the low 16 bits of the CRC-32 of the header so far
        if (len - pos < 2) return ALZ_E_STREAM;
        const uint32_t want = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
        if ((kCrc.of(src + start, pos - start) & 0xFFFFu) != want) return ALZ_E_CHECKSUM;
        pos += 2;
    }
    return ALZ_OK;
}

// RFC 1952: members (header, body, CRC-32 and ISIZE of the member's output) while the next two bytes are 1F 8B
int gzip_file(alz_ctx* ctx, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, const Outcome& o) {
    size_t pos = 0, out = 0;
    for (bool first = true;; first = false) {
        if (!first && !(len - pos >= 2 && src[pos] == 0x1F && src[pos + 1] == 0x8B)) break;   // anything else behind a member ends decoding
        const int hrc = gzip_header(src, len, pos);
        if (hrc == ALZ_E_STREAM) return o.stream(ALZ_ST_INPUT_TRUNCATED, out, len);
        if (hrc) return o.end(hrc, ALZ_ST_OK, out, pos);
        alz_result r;
        if (int rc = body(ctx, src, len, pos, dst, cap, out, o.measure, &r)) return rc;
        const size_t mstart = out;
        out += r.dst_len;
        if (r.status != ALZ_ST_OK) return o.stream(r.status, out, pos + (size_t)r.src_used);
        pos += (size_t)r.src_used;
        if (len - pos < 8) return o.stream(ALZ_ST_INPUT_TRUNCATED, out, len);
        const bool crc_ok = o.measure || le32(src + pos) == kCrc.of(dst + mstart, r.dst_len);
        if (!crc_ok || le32(src + pos + 4) != r.dst_len) return o.end(ALZ_E_CHECKSUM, ALZ_ST_OK, out, pos + 8);   // (a stream holds fewer than 2^32 bytes: ISIZE is its length)
        pos += 8;
    }
    return o.end(ALZ_OK, ALZ_ST_OK, out, len);                                  // source.Position = source.Length  GZip.cs:33
}

typedef int (*file_fn)(alz_ctx*, const uint8_t*, size_t, uint8_t*, size_t, const Outcome&);
int run(file_fn f, alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t cap, bool measure,
        size_t* dst_len, size_t* src_used, int32_t* status) {
    if ((src_len && !src) || (!measure && cap && !dst)) return ALZ_E_INVALID;
    const Outcome o = {dst_len, src_used, status, measure};
    (void)o.end(0, ALZ_ST_OK, 0, 0);
    return f(ctx, src, src_len, measure ? nullptr : dst, cap, o);
}

}   // namespace

// IsMatchStatic  ZLib.cs:26-27: Position + 4 < Length && CheckZlibHeaderAndFirstBlock(Peek<uint>())  :52-76
int alz_zlib_is_match(const uint8_t* src, size_t src_len) {
    if (!src || !(src_len > 4)) return 0;
    const uint32_t cmf = src[0], flg = src[1], d1 = src[2], d2 = src[3];
    if ((cmf & 0x0Fu) != 8u) return 0;                                          // CM != deflate
    if (((cmf >> 4) & 0x0Fu) > 7u) return 0;                                    // CINFO > 7
    if ((cmf * 256u + flg) % 31u != 0u) return 0;
    const uint32_t btype = (d1 >> 1) & 3u;
    if (btype == 3u) return 0;
    if (btype == 0u) {                                                          // as written: LEN is read from the first two data bytes  :70
        const uint16_t len = (uint16_t)(d1 | (d2 << 8)), nlen = (uint16_t)~len;
        if ((len ^ nlen) != 0xFFFF) return 0;
        if (len == 0) return 0;
    }
    return 1;
}

// IsMatchStatic  GZip.cs:25-26: Position + 8 < Length && the bytes 1F 8B 08
int alz_gzip_is_match(const uint8_t* src, size_t src_len) {
    return src && src_len > 8 && src[0] == 0x1F && src[1] == 0x8B && src[2] == 0x08;
}

int alz_zlib_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status) {
    return run(zlib_file, ctx, src, src_len, dst, dst_cap, false, dst_len, src_used, status);
}
int alz_gzip_decompress(alz_ctx* ctx, const uint8_t* src, size_t src_len, uint8_t* dst, size_t dst_cap,
                        size_t* dst_len, size_t* src_used, int32_t* status) {
    return run(gzip_file, ctx, src, src_len, dst, dst_cap, false, dst_len, src_used, status);
}
int alz_zlib_measure(alz_ctx* ctx, const uint8_t* src, size_t src_len, size_t size_limit,
                     size_t* size_out, size_t* src_used, int32_t* status) {
    return run(zlib_file, ctx, src, src_len, nullptr, size_limit, true, size_out, src_used, status);
}
int alz_gzip_measure(alz_ctx* ctx, const uint8_t* src, size_t src_len, size_t size_limit,
                     size_t* size_out, size_t* src_used, int32_t* status) {
    return run(gzip_file, ctx, src, src_len, nullptr, size_limit, true, size_out, src_used, status);
}
