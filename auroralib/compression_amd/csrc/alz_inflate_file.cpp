// alz_inflate_file.cpp -- the ZLib and GZip classes of the reference (Formats/Common/ZLib.cs, GZip.cs) over alz_inflate_decode_batch /
// alz_inflate_measure_batch: IsMatch, Decompress(Stream, Stream) and the size of a file without decoding it.  The reference hands both
// bodies to the BCL, so the framing is RFC 1950 (zlib) and RFC 1952 (gzip) as zlib reads them; checksums are computed here, on the host,
// over the downloaded output.  Pure host code on the public ABI.
#include <cstring>

#include "auroralz.h"
#include "alz_zfile.h"

namespace {

using namespace alz_zframe;                                                    // header walks, trailer fields and the host checksums: shared with alz_zfile.cpp

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
    if (int rc = zlib_header(src, len)) return rc;
    alz_result r;
    if (int rc = body(ctx, src, len, 2, dst, cap, 0, o.measure, &r)) return rc;
    if (r.status != ALZ_ST_OK) return o.stream(r.status, r.dst_len, 2 + (size_t)r.src_used);
    const size_t pos = 2 + (size_t)r.src_used;
    if (len - pos < 4) return o.stream(ALZ_ST_INPUT_TRUNCATED, r.dst_len, len);
    if (!o.measure && !zlib_trailer_ok(src + pos, adler32(dst, r.dst_len))) return o.end(ALZ_E_CHECKSUM, ALZ_ST_OK, r.dst_len, pos + 4);
    return o.end(ALZ_OK, ALZ_ST_OK, r.dst_len, pos + 4);
}

// RFC 1952: members (header, body, CRC-32 and ISIZE of the member's output) while the next two bytes are 1F 8B
int gzip_file(alz_ctx* ctx, const uint8_t* src, size_t len, uint8_t* dst, size_t cap, const Outcome& o) {
    size_t pos = 0, out = 0;
    for (bool first = true;; first = false) {
        if (!first && !gzip_member_follows(src, len, pos)) break;                              // anything else behind a member ends decoding
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
        const uint32_t crc = o.measure ? 0u : crc32().of(dst + mstart, r.dst_len);
        if (!gzip_trailer_ok(src + pos, o.measure ? nullptr : &crc, r.dst_len)) return o.end(ALZ_E_CHECKSUM, ALZ_ST_OK, out, pos + 8);   // (a stream holds fewer than 2^32 bytes: ISIZE is its length)
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
    return zlib_is_match(src, src_len) ? 1 : 0;                                 // (alz_zfile.h: the wrapped-file walks ask the same question)
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
