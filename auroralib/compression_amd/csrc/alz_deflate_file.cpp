// alz_deflate_file.cpp -- ZLib (RFC 1950) and GZip (RFC 1952) files WRITTEN over alz_deflate_encode_batch_device: one file
// (alz_deflate_file_compress) and a whole set in one call (alz_deflate_file_compress_batch).  The bodies are the library's own DEFLATE
// encoder (alz_inflate.hip); the reference hands these two classes' Compress to the BCL, so there are no managed bytes to match and the
// framing is what zlib writes: the level byte of the zlib header, XFL of the gzip header, Adler-32 / CRC-32 of the INPUT.  The batch is
// differential against the single-file call: both size a body's slot by the same rule and the encoder's bytes do not depend on the batch.
// Pure host code on the public ABI plus the range-copy kernel (alz_xxh32.h).
#include <cstring>
#include <vector>

#include "auroralz.h"
#include "alz_file_batch.h"
#include "alz_xxh32.h"
#include "alz_zfile.h"

namespace {

using namespace alz_file_batch;
using alz_zframe::adler32;
using alz_zframe::crc32;

const size_t kGzipHeader = 10;
inline size_t head_of(uint32_t kind) { return kind == ALZ_ZFILE_ZLIB ? alz_zframe::kZlibHeader : kGzipHeader; }
inline size_t tail_of(uint32_t kind) { return kind == ALZ_ZFILE_ZLIB ? alz_zframe::kZlibTrailer : alz_zframe::kGzipTrailer; }
inline bool settings_ok(int level, uint32_t flags) { return level >= 0 && level <= 9 && !(flags & ~ALZ_DEFLATE_FIXED); }

size_t write_head(uint32_t kind, int level, uint8_t* p) {
    if (kind == ALZ_ZFILE_ZLIB) {                                               // CMF 78: deflate, 32 KiB; FLG: FLEVEL and the check bits
        p[0] = 0x78; p[1] = level <= 1 ? 0x01 : level <= 5 ? 0x5E : level == 6 ? 0x9C : 0xDA;
        return 2;
    }
    const uint8_t h[10] = {0x1F, 0x8B, 0x08, 0x00, 0, 0, 0, 0, (uint8_t)(level <= 1 ? 4 : level == 9 ? 2 : 0), 0x03};
    memcpy(p, h, 10);
    return 10;
}
size_t write_tail(uint32_t kind, uint32_t sum, uint32_t src_len, uint8_t* p) {
    if (kind == ALZ_ZFILE_ZLIB) { p[0] = (uint8_t)(sum >> 24); p[1] = (uint8_t)(sum >> 16); p[2] = (uint8_t)(sum >> 8); p[3] = (uint8_t)sum; return 4; }
    for (int k = 0; k < 4; k++) { p[k] = (uint8_t)(sum >> (8 * k)); p[4 + k] = (uint8_t)(src_len >> (8 * k)); }
    return 8;
}

// what a file is refused for before anything is encoded, and the capacity of its body's slot: both calls judge by this
int open_file(uint32_t kind, size_t src_len, size_t dst_cap, size_t* body_cap) {
    if (src_len >= 0x7FFFFF00ull) return ALZ_E_UNSUPPORTED;
    const size_t over = head_of(kind) + tail_of(kind);
    if (dst_cap < over) return ALZ_E_NOMEM;
    const size_t bound = alz_deflate_bound(src_len);
    *body_cap = dst_cap - over < bound ? dst_cap - over : bound;
    return ALZ_OK;
}

}   // namespace

extern "C" {

size_t alz_deflate_file_bound(uint32_t kind, size_t src_len) {
    if (kind > ALZ_ZFILE_GZIP) return 0;
    return alz_deflate_bound(src_len) + head_of(kind) + tail_of(kind);
}

int alz_deflate_file_compress(alz_ctx* ctx, uint32_t kind, int level, uint32_t flags, const uint8_t* src, size_t src_len,
                              uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    if (dst_len) *dst_len = 0;
    if (!ctx || kind > ALZ_ZFILE_GZIP || !settings_ok(level, flags) || (src_len && !src) || (dst_cap && !dst)) return ALZ_E_INVALID;
    size_t body_cap = 0;
    if (int rc = open_file(kind, src_len, dst_cap, &body_cap)) return rc;
    DeviceBuffer d_src(ctx), d_dst(ctx);
    int rc;
    if ((rc = d_src.alloc(src_len)) || (rc = d_dst.alloc(body_cap))) return rc;
    if (src_len && (rc = alz_memcpy_h2d(ctx, d_src.p, src, src_len))) return rc;
    alz_stream s; memset(&s, 0, sizeof(s));
    s.src_len = (uint32_t)src_len; s.dst_cap = (uint32_t)body_cap;
    alz_result r; memset(&r, 0, sizeof(r));
    if ((rc = alz_deflate_encode_batch_device(ctx, level, flags, 1, (const uint8_t*)d_src.p, src_len, &s, (uint8_t*)d_dst.p, body_cap, &r))) return rc;
    if (r.status != ALZ_ST_OK) return ALZ_E_NOMEM;
    const size_t h = write_head(kind, level, dst);
    if (r.dst_len && (rc = alz_memcpy_d2h(ctx, dst + h, d_dst.p, r.dst_len))) return rc;
    const uint32_t sum = kind == ALZ_ZFILE_ZLIB ? adler32(src, src_len) : crc32().of(src, src_len);
    const size_t t = write_tail(kind, sum, (uint32_t)src_len, dst + h + r.dst_len);
    if (dst_len) *dst_len = h + r.dst_len + t;
    return ALZ_OK;
}

int alz_deflate_file_compress_batch(alz_ctx* ctx, int level, uint32_t flags, uint32_t n, const uint8_t* src_base, size_t src_bytes,
                                    const alz_stream* files, uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, true, [](uint32_t kind) { return kind <= ALZ_ZFILE_GZIP; })) return rc;
    if (!settings_ok(level, flags)) return ALZ_E_INVALID;
    if (n == 0) return ALZ_OK;
    // ---- layout: [ source | >= 64 bytes ][ a slot per body ][ the header and trailer bytes ]
    const uint64_t src_al = ((uint64_t)src_bytes + 64 + 255) & ~255ull;
    std::vector<alz_stream> ss; std::vector<uint32_t> who;
    uint64_t slot_at = src_al, dlo = ~0ull, dhi = 0;
    for (uint32_t i = 0; i < n; i++) {
        size_t body_cap = 0;
        results[i] = alz_file_result{open_file(files[i].format, files[i].src_len, files[i].dst_cap, &body_cap), ALZ_ST_OK, 0, 0};
        if (results[i].rc != ALZ_OK) continue;
        alz_stream s; memset(&s, 0, sizeof(s));
        s.src_off = files[i].src_off; s.src_len = files[i].src_len; s.dst_off = slot_at; s.dst_cap = (uint32_t)body_cap;
        slot_at += ((uint64_t)body_cap + 15) & ~15ull;
        ss.push_back(s); who.push_back(i);
        dlo = std::min<uint64_t>(dlo, files[i].dst_off); dhi = std::max<uint64_t>(dhi, files[i].dst_off + files[i].dst_cap);
    }
    const uint32_t m = (uint32_t)ss.size();
    if (m == 0) return ALZ_OK;                                                  // every file was refused: nothing for the GPU
    const uint64_t table_at = slot_at, all = table_at + (uint64_t)m * 32;
    DeviceBuffer d_all(ctx), d_img(ctx);
    int rc;
    if ((rc = d_all.alloc((size_t)all))) return rc;
    uint8_t* da = (uint8_t*)d_all.p;
    if (src_bytes && (rc = alz_memcpy_h2d(ctx, da, src_base, src_bytes))) return rc;
    // ---- all bodies as one encode; the raw inputs summed where they lie, one batch per kind present
    std::vector<alz_result> rs(m);
    if ((rc = alz_deflate_encode_batch_device(ctx, level, flags, m, da, (size_t)src_al, ss.data(), da, (size_t)table_at, rs.data()))) return rc;
    std::vector<alz_stream> ranges[2]; std::vector<uint32_t> sums[2], slot(m, 0);
    for (uint32_t j = 0; j < m; j++) {
        if (rs[j].status != ALZ_ST_OK) continue;
        const uint32_t kind = files[who[j]].format == ALZ_ZFILE_ZLIB ? ALZ_CK_ADLER32 : ALZ_CK_CRC32;
        slot[j] = (uint32_t)ranges[kind].size();
        ranges[kind].push_back(ss[j]);
    }
    for (uint32_t kind = 0; kind < 2; kind++) {
        sums[kind].assign(ranges[kind].size(), 0);
        if (ranges[kind].empty()) continue;
        if ((rc = alz_checksum_batch_device(ctx, kind, (uint32_t)ranges[kind].size(), da, (size_t)src_al, ranges[kind].data(), sums[kind].data()))) return rc;
    }
    // ---- the file images: header, body, trailer -- assembled in HBM by one range copy, downloaded once
    std::vector<alz_copy_range> copies; std::vector<uint8_t> table((size_t)m * 32, 0);
    for (uint32_t j = 0; j < m; j++) {
        const uint32_t i = who[j], kind = files[i].format;
        if (rs[j].status != ALZ_ST_OK) { results[i].rc = ALZ_E_NOMEM; continue; }
        const uint32_t sum = sums[kind == ALZ_ZFILE_ZLIB ? ALZ_CK_ADLER32 : ALZ_CK_CRC32][slot[j]];
        uint8_t* t = table.data() + (size_t)j * 32;
        const size_t h = write_head(kind, level, t), tl = write_tail(kind, sum, files[i].src_len, t + 16);
        const uint64_t img = files[i].dst_off - dlo;
        copies.push_back(alz_copy_range{table_at + (uint64_t)j * 32, img, (uint32_t)h, 0});
        if (rs[j].dst_len) copies.push_back(alz_copy_range{ss[j].dst_off, img + h, rs[j].dst_len, 0});
        copies.push_back(alz_copy_range{table_at + (uint64_t)j * 32 + 16, img + h + rs[j].dst_len, (uint32_t)tl, 0});
        results[i].dst_len = (uint32_t)(h + rs[j].dst_len + tl); results[i].src_used = files[i].src_len;
    }
    if (copies.empty()) return ALZ_OK;
    if ((rc = alz_memcpy_h2d(ctx, da + table_at, table.data(), table.size()))) return rc;
    if ((rc = d_img.alloc((size_t)(dhi - dlo)))) return rc;
    if ((rc = alz_host_range_copy(ctx, (uint32_t)copies.size(), copies.data(), da, (size_t)all, (uint8_t*)d_img.p, (size_t)(dhi - dlo)))) return rc;
    std::vector<alz_stream> placed(files, files + n);
    for (alz_stream& f : placed) f.dst_off = f.dst_off >= dlo ? f.dst_off - dlo : 0;   // (a refused file may lie in front of dlo: it has no bytes)
    return download(ctx, n, placed.data(), results, d_img.p, dst_base + dlo);
}

}   // extern "C"
