// alz_wfile.cpp -- the wrapped files: RLHudson and the seven wrapper classes of the .Extended assembly (alz_wfile_*; include/auroralz.h has
// the layouts and the rules).  The walks are alz_zfile.h's (alz_wframe); this file runs what they return: the source to the device once, all
// parts of all files of a call as one batch per body kind, the outputs downloaded once.  The single-file call is a batch of one, so the
// differential contract of alz_wfile_decode_batch holds by construction.  Pure host code on the public ABI.
#include <algorithm>
#include <cstring>
#include <vector>

#include "auroralz.h"
#include "alz_file_batch.h"
#include "alz_zfile.h"

namespace {

using namespace alz_wframe;
using namespace alz_file_batch;
using alz_zframe::kMaxCap;
using alz_zframe::kZlibHeader;
using alz_zframe::kZlibTrailer;

bool bounded_kind(uint32_t kind) { return kind == ALZ_WF_ASURAZLB || kind == ALZ_WF_ZLB || kind == ALZ_WF_HWGZ; }
bool exact_size_kind(uint32_t kind) { return kind != ALZ_WF_RAREZIP && kind != ALZ_WF_RLHUDSON; }

struct Part { alz_wfile_part p; uint32_t file; size_t out_off; alz_result r; uint32_t sum; bool has_sum, run; };
struct File {
    std::vector<alz_wfile_part> parts; uint32_t stated = 0, flags = 0, first = 0;   // first: index of its first Part
    bool done = false;                                                          // its result is final
};

void finish(alz_file_result& r, File& f, int rc, int32_t status, size_t out, size_t used) {
    r.rc = rc; r.status = status; r.dst_len = (uint32_t)out; r.src_used = (uint32_t)used; f.done = true;
}

// the stated size against what an otherwise successful decode delivered: '!=' for six kinds, '>' for RareZip and RLHudson
void close_file(alz_file_result& r, File& f, const alz_stream& file, size_t out, size_t used) {
    const bool mismatch = exact_size_kind(file.format) ? out != f.stated : out > f.stated;
    finish(r, f, mismatch ? ALZ_E_STREAM : ALZ_OK, mismatch ? ALZ_ST_OUTPUT_SIZE_MISMATCH : ALZ_ST_OK, out, used);
}

alz_stream stream_of(uint64_t src_off, uint32_t src_len, uint64_t dst_off, size_t cap) {
    alz_stream s; memset(&s, 0, sizeof(s));
    s.src_off = src_off; s.src_len = src_len; s.dst_off = dst_off; s.dst_cap = cap > kMaxCap ? kMaxCap : (uint32_t)cap;
    return s;
}

// the keystream of a call: drawn once, up to the longest encrypted payload
void sszl_keystream(std::vector<uint32_t>& ks, size_t bytes) {
    SszlTwister mt;
    ks.resize((bytes + 3) / 4);
    for (uint32_t& w : ks) w = mt.next();
}

int decode_files(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, uint8_t* dst_base, size_t dst_bytes,
                 alz_file_result* results) {
    std::vector<File> fs(n);
    std::vector<Part> ps;
    size_t longest_enc = 0;
    // ---- the walks
    for (uint32_t i = 0; i < n; i++) {
        const alz_stream& f = files[i];
        const uint8_t* src = src_base + f.src_off;
        alz_container_options opt; memset(&opt, 0, sizeof(opt)); opt.big_endian = f.aux0 & 1u;
        results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
        uint32_t np = 0;
        int rc = walk(f.format, &opt, src, f.src_len, nullptr, 0, &np, &fs[i].stated, &fs[i].flags);
        if (rc == ALZ_E_INVALID && np) {
            fs[i].parts.resize(np);
            rc = walk(f.format, &opt, src, f.src_len, fs[i].parts.data(), np, &np, &fs[i].stated, &fs[i].flags);
        }
        if (rc == ALZ_E_STREAM) { finish(results[i], fs[i], ALZ_E_STREAM, ALZ_ST_INPUT_TRUNCATED, 0, f.src_len); continue; }
        if (rc) { finish(results[i], fs[i], rc, ALZ_ST_OK, 0, 0); continue; }
        fs[i].first = (uint32_t)ps.size();
        for (const alz_wfile_part& p : fs[i].parts) ps.push_back(Part{p, i, 0, alz_result{0, 0, 0, 0}, 0, false, false});
        if (f.format == ALZ_WF_SSZL && (fs[i].flags & ALZ_SSZL_ENCRYPTED)) longest_enc = std::max(longest_enc, (size_t)f.src_len - 20);
    }
    if (ps.empty()) {                                                           // every file ended in its header or has no chunk: nothing for the GPU, no context needed
        for (uint32_t i = 0; i < n; i++)                                        // (a ZLWF file of no chunks: its stated size is still checked)
            if (!fs[i].done) close_file(results[i], fs[i], files[i], 0, files[i].src_len);
        return ALZ_OK;
    }
    if (!ctx) return ALZ_E_INVALID;

    // ---- the source, XORed where a file says so, to the device once
    std::vector<uint8_t> staged; std::vector<uint32_t> ks;
    const uint8_t* host_src = src_base;
    if (longest_enc) {
        sszl_keystream(ks, longest_enc);
        staged.assign(src_base, src_base + src_bytes);
        for (uint32_t i = 0; i < n; i++)
            if (!fs[i].done && files[i].format == ALZ_WF_SSZL && (fs[i].flags & ALZ_SSZL_ENCRYPTED))
                sszl_xor(staged.data() + files[i].src_off + 20, (size_t)files[i].src_len - 20, ks.data());
        host_src = staged.data();
    }
    DeviceBuffer d_src(ctx), d_dst(ctx);
    int rc;
    if ((rc = d_src.alloc(src_bytes + 64)) || (rc = alz_memcpy_h2d(ctx, d_src.p, host_src, src_bytes))) return rc;
    if ((rc = d_dst.alloc(dst_bytes + 64))) return rc;
    const uint8_t* ds = (const uint8_t*)d_src.p; uint8_t* dd = (uint8_t*)d_dst.p;

    // ---- zlib headers; the chunks of the HWGZ files measured, so that every part knows where its output goes
    std::vector<alz_stream> ss; std::vector<alz_result> rs; std::vector<uint32_t> who;
    std::vector<int> hdr_rc(ps.size(), ALZ_OK);
    for (size_t k = 0; k < ps.size(); k++) {
        if (ps[k].p.body != ALZ_WB_ZLIB) continue;
        hdr_rc[k] = alz_zframe::zlib_header(host_src + files[ps[k].file].src_off + ps[k].p.src_off, ps[k].p.src_len);
        if (!hdr_rc[k] && files[ps[k].file].format == ALZ_WF_HWGZ) {
            who.push_back((uint32_t)k);
            ss.push_back(stream_of(files[ps[k].file].src_off + ps[k].p.src_off + kZlibHeader, ps[k].p.src_len - (uint32_t)kZlibHeader, 0, kMaxCap));
        }
    }
    std::vector<uint32_t> measured(ps.size(), 0);
    if (!ss.empty()) {
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if ((rc = alz_inflate_measure_batch_device(ctx, (uint32_t)ss.size(), ds, src_bytes, ss.data(), rs.data()))) return rc;
        for (size_t j = 0; j < who.size(); j++) measured[who[j]] = rs[j].dst_len;
    }
    // a part's destination: the decoded sizes in front of it.  A part behind one that cannot succeed is not run.
    for (uint32_t i = 0; i < n; i++) {
        if (fs[i].done) continue;
        size_t out = 0; bool stop = false;
        for (size_t k = fs[i].first; k < fs[i].first + fs[i].parts.size(); k++) {
            ps[k].out_off = out; ps[k].run = !stop && !hdr_rc[k];
            if (hdr_rc[k]) stop = true;
            const size_t room = out < files[i].dst_cap ? files[i].dst_cap - out : 0;
            size_t len = files[i].format == ALZ_WF_HWGZ ? measured[k] : ps[k].p.dst_len;      // (single-part kinds: nothing follows)
            if (len > room) { len = room; stop = true; }                        // this part meets dst_cap: nothing behind it runs
            out += len;
        }
    }

    // ---- one batch per body kind
    auto room_of = [&](const Part& p) { const size_t cap = files[p.file].dst_cap; return p.out_off < cap ? cap - p.out_off : 0; };
    auto run_kind = [&](auto accepts, auto make, auto call) -> int {
        ss.clear(); who.clear();
        for (size_t k = 0; k < ps.size(); k++) if (ps[k].run && accepts(ps[k])) { who.push_back((uint32_t)k); ss.push_back(make(ps[k])); }
        if (ss.empty()) return ALZ_OK;
        rs.assign(ss.size(), alz_result{0, 0, 0, 0});
        if (int e = call()) return e;
        for (size_t j = 0; j < who.size(); j++) ps[who[j]].r = rs[j];
        return ALZ_OK;
    };
    auto src_at = [&](const Part& p) { return files[p.file].src_off + p.p.src_off; };
    auto dst_at = [&](const Part& p) { return files[p.file].dst_off + p.out_off; };
    // DEFLATE: the zlib bodies behind their two header bytes and RareZip's raw streams
    if ((rc = run_kind([](const Part& p) { return p.p.body == ALZ_WB_ZLIB || p.p.body == ALZ_WB_DEFLATE; },
                       [&](const Part& p) { const uint32_t h = p.p.body == ALZ_WB_ZLIB ? (uint32_t)kZlibHeader : 0u;
                                            return stream_of(src_at(p) + h, p.p.src_len - h, dst_at(p), room_of(p)); },
                       [&] { return alz_inflate_decode_batch_device(ctx, (uint32_t)ss.size(), ds, src_bytes, ss.data(), dd, dst_bytes, rs.data()); }))) return rc;
    {   // ... and the Adler-32 of every zlib output that will meet a whole trailer, summed where it lies
        std::vector<alz_stream> ranges; std::vector<uint32_t> owner;
        for (size_t k = 0; k < ps.size(); k++) {
            const Part& p = ps[k];
            if (!p.run || p.p.body != ALZ_WB_ZLIB || p.r.status != ALZ_ST_OK) continue;
            if ((size_t)p.p.src_len - kZlibHeader - p.r.src_used < kZlibTrailer) continue;
            ranges.push_back(stream_of(dst_at(p), p.r.dst_len, 0, 0)); owner.push_back((uint32_t)k);
        }
        if (!ranges.empty()) {
            std::vector<uint32_t> sums(ranges.size(), 0);
            if ((rc = alz_checksum_batch_device(ctx, ALZ_CK_ADLER32, (uint32_t)ranges.size(), dd, dst_bytes, ranges.data(), sums.data()))) return rc;
            for (size_t j = 0; j < owner.size(); j++) { ps[owner[j]].sum = sums[j]; ps[owner[j]].has_sum = true; }
        }
    }
    // WFLZ bodies: one plan.  A chunk decodes into the size it states and no further, so that a body that runs past it never writes where its
    // neighbour of the same plan writes (the two would race); such a chunk ends in OUTPUT_CAPACITY here and is a size mismatch below.
    if ((rc = run_kind([](const Part& p) { return p.p.body == ALZ_WB_WFLZ || p.p.body == ALZ_WB_WFLZ_BE; },
                       [&](const Part& p) { alz_stream s = stream_of(src_at(p), p.p.src_len, dst_at(p), std::min<size_t>(room_of(p), p.p.dst_len));
                                            s.format = p.p.body == ALZ_WB_WFLZ_BE ? ALZ_FMT_WFLZ_BE : ALZ_FMT_WFLZ; return s; },
                       [&] { return run_plan(ctx, ss, rs, ds, dd); }))) return rc;
    // RLHudson bodies
    if ((rc = run_kind([](const Part& p) { return p.p.body == ALZ_WB_RLHUDSON; },
                       [&](const Part& p) { alz_stream s = stream_of(src_at(p), p.p.src_len, dst_at(p), room_of(p)); s.decom_len = p.p.dst_len; return s; },
                       [&] { return alz_rlhudson_decode_batch_device(ctx, (uint32_t)ss.size(), ds, src_bytes, ss.data(), dd, dst_bytes, rs.data()); }))) return rc;
    // plain bytes: copied
    for (Part& p : ps) {
        if (!p.run || p.p.body != ALZ_WB_PLAIN) continue;
        const size_t room = room_of(p), take = std::min<size_t>(p.p.src_len, room);
        if (take && (rc = alz_memcpy_h2d(ctx, dd + dst_at(p), host_src + src_at(p), take))) return rc;
        p.r.dst_len = (uint32_t)take; p.r.src_used = (uint32_t)take;
        p.r.status = p.p.src_len > room ? ALZ_ST_OUTPUT_CAPACITY : ALZ_ST_OK;
    }
    // gzip payloads (SSZL only): the batch that reads such files, on the decrypted bytes, straight into the caller's destination
    std::vector<uint32_t> gz_file; std::vector<alz_file_result> gz_res;
    {
        std::vector<alz_stream> gz;
        for (const Part& p : ps) {
            if (!p.run || p.p.body != ALZ_WB_GZIP) continue;
            alz_stream s = stream_of(src_at(p), p.p.src_len, dst_at(p), room_of(p)); s.format = ALZ_ZFILE_GZIP;
            gz.push_back(s); gz_file.push_back(p.file);
        }
        gz_res.resize(gz.size());
        if (!gz.empty() && (rc = alz_zfile_decode_batch(ctx, (uint32_t)gz.size(), host_src, src_bytes, gz.data(), dst_base, dst_bytes, gz_res.data()))) return rc;
    }

    // ---- every file's result from its parts
    for (uint32_t i = 0; i < n; i++) {
        File& f = fs[i];
        if (f.done) continue;
        const uint32_t kind = files[i].format, len = files[i].src_len;
        size_t out = 0, used = 0;
        for (size_t k = f.first; k < f.first + f.parts.size() && !f.done; k++) {
            const Part& p = ps[k];
            if (p.p.body == ALZ_WB_GZIP) break;                                 // (below)
            if (hdr_rc[k]) { finish(results[i], f, hdr_rc[k], ALZ_ST_OK, out, p.p.src_off); break; }
            const size_t hdr = p.p.body == ALZ_WB_ZLIB ? kZlibHeader : 0;
            out += p.r.dst_len;
            if ((p.p.body == ALZ_WB_WFLZ || p.p.body == ALZ_WB_WFLZ_BE) && p.r.status == ALZ_ST_OUTPUT_CAPACITY && room_of(p) > p.p.dst_len) {
                finish(results[i], f, ALZ_E_STREAM, ALZ_ST_OUTPUT_SIZE_MISMATCH, out, p.p.src_off + p.r.src_used); break;   // the body runs past the size it states: WFLZ.cs:82-85, the stated bytes delivered
            }
            if (p.r.status != ALZ_ST_OK) { finish(results[i], f, ALZ_E_STREAM, p.r.status, out, p.r.status == ALZ_ST_INPUT_TRUNCATED && !bounded_kind(kind) ? len : p.p.src_off + hdr + p.r.src_used); break; }
            used = p.p.src_off + hdr + p.r.src_used;
            if (p.p.body == ALZ_WB_ZLIB) {
                const size_t left = p.p.src_len - hdr - p.r.src_used;
                if (left >= kZlibTrailer) {
                    used += kZlibTrailer;
                    const uint8_t* t = host_src + files[i].src_off + p.p.src_off + hdr + p.r.src_used;
                    if (!alz_zframe::zlib_trailer_ok(t, p.sum)) { finish(results[i], f, ALZ_E_CHECKSUM, ALZ_ST_OK, out, used); break; }
                } else if (!bounded_kind(kind)) { finish(results[i], f, ALZ_E_STREAM, ALZ_ST_INPUT_TRUNCATED, out, len); break; }   // as alz_zlib_decompress
                else used += left;                                              // a bounded body whose trailer is cut: OK, unverified
            }
            if ((p.p.body == ALZ_WB_WFLZ || p.p.body == ALZ_WB_WFLZ_BE) && p.r.dst_len != p.p.dst_len) {   // WFLZ.cs:82-85
                finish(results[i], f, ALZ_E_STREAM, ALZ_ST_OUTPUT_SIZE_MISMATCH, out, used); break;
            }
        }
        if (f.done) continue;
        if (kind == ALZ_WF_SSZL || kind == ALZ_WF_ZLWF) used = len;             // the payload is read to its end; the chunks lie where the table says
        if (kind == ALZ_WF_HWGZ) used = (size_t)std::min<uint64_t>(len, align_up(used, 128));   // Align(128) behind every chunk  HWGZ.cs:78
        if (kind == ALZ_WF_RAREZIP && out < f.stated) {                         // SetLength: zeros up to the stated size
            const size_t end = std::min<size_t>(f.stated, files[i].dst_cap);
            if (end > out && (rc = alz_memset_d(ctx, dd + files[i].dst_off + out, 0, end - out))) return rc;
            out = end;
        }
        close_file(results[i], f, files[i], out, used);
    }
    for (size_t j = 0; j < gz_file.size(); j++) {                               // gzip payloads: alz_gzip_decompress's result behind the 20-byte header
        const uint32_t i = gz_file[j];
        alz_file_result r = gz_res[j];
        r.src_used += 20;
        if (r.rc == ALZ_OK && r.dst_len != fs[i].stated) { r.rc = ALZ_E_STREAM; r.status = ALZ_ST_OUTPUT_SIZE_MISMATCH; }
        results[i] = r;
    }
    // ---- the outputs, once (the gzip payloads are in place already)
    std::vector<alz_file_result> dl(results, results + n);
    for (uint32_t i : gz_file) dl[i].dst_len = 0;
    return download(ctx, n, files, dl.data(), d_dst.p, dst_base);
}

void be32w(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }
void le32w(uint8_t* p, uint32_t v) { p[3] = (uint8_t)(v >> 24); p[2] = (uint8_t)(v >> 16); p[1] = (uint8_t)(v >> 8); p[0] = (uint8_t)v; }
void wr32(uint8_t* p, uint32_t v, bool big) { if (big) be32w(p, v); else le32w(p, v); }

uint32_t hwgz_chunk(const alz_container_options* opt) { return opt && opt->chunk_size ? opt->chunk_size : 0x10000u; }
uint32_t zlwf_block(const alz_container_options* opt) { return opt && opt->chunk_size ? opt->chunk_size : 0x400000u; }
uint32_t sszl_options(const alz_container_options* opt) { return opt && opt->variant ? opt->variant : (ALZ_SSZL_COMPRESSED | ALZ_SSZL_ENCRYPTED); }

}   // namespace

int alz_wfile_is_match(uint32_t kind, const uint8_t* src, size_t len) { return is_match(kind, src, len); }

int alz_wfile_decompressed_size(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, uint32_t* size_out) {
    return decompressed_size(kind, opt, src, len, size_out);
}

int alz_wfile_walk(uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len, alz_wfile_part* parts, uint32_t cap,
                   uint32_t* n_parts, uint32_t* stated_size, uint32_t* flags) {
    return walk(kind, opt, src, len, parts, cap, n_parts, stated_size, flags);
}

int alz_wfile_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                           uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, true, [](uint32_t format) { return format < ALZ_WF_COUNT; })) return rc;
    if (n == 0) return ALZ_OK;
    return decode_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results);
}

int alz_wfile_decompress(alz_ctx* ctx, uint32_t kind, const alz_container_options* opt, const uint8_t* src, size_t len,
                         uint8_t* dst, size_t dst_cap, size_t* dst_len, size_t* src_used, int32_t* status) {
    if (kind >= ALZ_WF_COUNT || (len && !src) || (dst_cap && !dst) || len > kMaxCap) return ALZ_E_INVALID;
    alz_stream f = stream_of(0, (uint32_t)len, 0, dst_cap);
    f.format = kind; f.aux0 = opt && opt->big_endian ? 1u : 0u;
    alz_file_result r{ALZ_OK, ALZ_ST_OK, 0, 0};
    const int rc = decode_files(ctx, 1, src, len, &f, dst, f.dst_cap, &r);      // (a NULL ctx is refused there, once a body must be decoded)
    if (dst_len) *dst_len = rc ? 0 : r.dst_len;
    if (src_used) *src_used = rc ? 0 : r.src_used;
    if (status) *status = rc ? ALZ_ST_OK : r.status;
    return rc ? rc : r.rc;
}

size_t alz_wfile_compress_bound(uint32_t kind, const alz_container_options* opt, size_t src_len) {
    switch (kind) {
    case ALZ_WF_RLHUDSON: return 8 + alz_rlhudson_encode_bound(src_len);
    case ALZ_WF_ZLWF: { const size_t b = zlwf_block(opt), c = (src_len + b - 1) / b; return 32 + 4 * c + alz_container_compress_bound(ALZ_C_WFLZ, src_len) + c * (alz_container_compress_bound(ALZ_C_WFLZ, 0) + 32); }
    case ALZ_WF_HWGZ: { const size_t b = hwgz_chunk(opt), c = (src_len + b - 1) / b; return 256 + 4 * c + c * (alz_deflate_file_bound(ALZ_ZFILE_ZLIB, b) + 4 + 128); }
    case ALZ_WF_RAREZIP: return 6 + alz_deflate_bound(src_len);
    default: return 32 + std::max(alz_deflate_file_bound(ALZ_ZFILE_GZIP, src_len), src_len);
    }
}

int alz_wfile_compress(alz_ctx* ctx, uint32_t kind, const alz_container_options* opt, const alz_settings* settings, int level, uint32_t flags,
                       const uint8_t* src, size_t len, uint8_t* dst, size_t dst_cap, size_t* dst_len) {
    if (dst_len) *dst_len = 0;
    if (kind >= ALZ_WF_COUNT || (len && !src) || !dst || !dst_len || len > 0x7FFFFF00u) return ALZ_E_INVALID;
    if (!ctx) return ALZ_E_INVALID;
    if (dst_cap < alz_wfile_compress_bound(kind, opt, len)) return ALZ_E_INVALID;
    const bool big = opt && opt->big_endian;
    size_t got = 0; int rc;
    auto zlib_at = [&](size_t at, uint32_t zkind) { return alz_deflate_file_compress(ctx, zkind, level, flags, src, len, dst + at, dst_cap - at, &got); };
    switch (kind) {
    case ALZ_WF_RLHUDSON: {                                                     // RLHudson.cs:46-52
        be32w(dst, (uint32_t)len); be32w(dst + 4, 5);
        alz_stream s = stream_of(0, (uint32_t)len, 8, dst_cap - 8); alz_result r{0, 0, 0, 0};
        if (len && (rc = alz_rlhudson_encode_batch(ctx, 1, src, len, &s, dst, dst_cap, &r))) return rc;
        if (len && r.status != ALZ_ST_OK) return ALZ_E_INVALID;
        *dst_len = 8 + (len ? r.dst_len : 0);
        return ALZ_OK;
    }
    case ALZ_WF_ZLWF: {                                                         // ZLWF.cs:98-144
        const size_t block = zlwf_block(opt), chunks = (len + block - 1) / block;
        alz_container_options wo; memset(&wo, 0, sizeof(wo)); wo.big_endian = big;
        memcpy(dst, "ZLWF", 4); wr32(dst + 8, (uint32_t)len, big); wr32(dst + 12, (uint32_t)chunks, big);
        size_t pos = 16 + 4 * chunks;
        for (size_t i = 0; i < chunks; i++) {
            while (pos & 15) dst[pos++] = 0;                                    // WriteAlign(0x10)
            wr32(dst + 16 + 4 * i, (uint32_t)pos, big);
            const size_t a = i * block, bl = std::min(block, len - a);
            if ((rc = alz_container_compress(ctx, ALZ_C_WFLZ, &wo, settings, src + a, bl, dst + pos, dst_cap - pos, &got))) return rc;
            pos += got;
        }
        while (pos & 15) dst[pos++] = 0;
        wr32(dst + 4, (uint32_t)(pos - 0x10), big);
        *dst_len = pos;
        return ALZ_OK;
    }
    case ALZ_WF_ASURAZLB:                                                       // AsuraZlb.cs:68-77
        memcpy(dst, "AsuraZlb", 8); le32w(dst + 8, 1); be32w(dst + 16, (uint32_t)len);
        if ((rc = zlib_at(20, ALZ_ZFILE_ZLIB))) return rc;
        be32w(dst + 12, (uint32_t)got);                                         // Length - start - 0x14
        *dst_len = 20 + got; return ALZ_OK;
    case ALZ_WF_ZLB:                                                            // ZLB.cs:73-89
        memcpy(dst, "ZLB\0", 4); be32w(dst + 4, 1); be32w(dst + 8, (uint32_t)len);
        if ((rc = zlib_at(16, ALZ_ZFILE_ZLIB))) return rc;
        be32w(dst + 12, (uint32_t)(16 + got - 0x14));                           // Length - start - 0x14 behind a 16-byte header: four short, as written
        *dst_len = 16 + got; return ALZ_OK;
    case ALZ_WF_MDF0:                                                           // MDF0.cs:57-62
        memcpy(dst, "mdf\0", 4); le32w(dst + 4, (uint32_t)len);
        if ((rc = zlib_at(8, ALZ_ZFILE_ZLIB))) return rc;
        *dst_len = 8 + got; return ALZ_OK;
    case ALZ_WF_RAREZIP: {                                                      // RareZip.cs:57-63
        dst[0] = 0x11; dst[1] = 0x72; be32w(dst + 2, (uint32_t)len);
        alz_stream s = stream_of(0, (uint32_t)len, 6, dst_cap - 6); alz_result r{0, 0, 0, 0};
        if ((rc = alz_deflate_encode_batch(ctx, level, flags, 1, src, len, &s, dst, dst_cap, &r))) return rc;
        if (r.status != ALZ_ST_OK) return ALZ_E_INVALID;
        *dst_len = 6 + r.dst_len; return ALZ_OK;
    }
    case ALZ_WF_SSZL: {                                                         // SSZL.cs:131-167
        const uint32_t o = sszl_options(opt);
        memcpy(dst, "SSZL", 4); le32w(dst + 4, 0x20101109u); le32w(dst + 8, (uint32_t)len); le32w(dst + 12, o & 0xFFFFFFFDu); le32w(dst + 16, 0);
        if (o & ALZ_SSZL_COMPRESSED) { if ((rc = zlib_at(20, (o & ALZ_SSZL_USE_GZIP) ? ALZ_ZFILE_GZIP : ALZ_ZFILE_ZLIB))) return rc; }
        else { if (len) memcpy(dst + 20, src, len); got = len; }
        if (o & ALZ_SSZL_ENCRYPTED) { std::vector<uint32_t> ks; sszl_keystream(ks, got); sszl_xor(dst + 20, got, ks.data()); }
        *dst_len = 20 + got; return ALZ_OK;
    }
    case ALZ_WF_HWGZ: {                                                         // HWGZ.cs:86-132
        const size_t chunk = hwgz_chunk(opt), count = (len + chunk - 1) / chunk, slot = (alz_deflate_file_bound(ALZ_ZFILE_ZLIB, chunk) + 15) / 16 * 16;
        wr32(dst, (uint32_t)chunk, big); wr32(dst + 4, (uint32_t)count, big); wr32(dst + 8, (uint32_t)len, big);
        std::vector<alz_stream> cs(count); std::vector<alz_file_result> cr(count); std::vector<uint8_t> tmp(count * slot + 64);
        for (size_t i = 0; i < count; i++) { cs[i] = stream_of(i * chunk, (uint32_t)std::min(chunk, len - i * chunk), i * slot, slot); cs[i].format = ALZ_ZFILE_ZLIB; }
        if (count && (rc = alz_deflate_file_compress_batch(ctx, level, flags, (uint32_t)count, src, len, cs.data(), tmp.data(), count * slot, cr.data()))) return rc;
        size_t pos = 12 + 4 * count;
        while (pos & 127) dst[pos++] = 0;                                       // WriteAlign(128)
        for (size_t i = 0; i < count; i++) {
            if (cr[i].rc) return cr[i].rc;
            wr32(dst + 12 + 4 * i, cr[i].dst_len + 4, big);                     // the table, every entry in the file's order
            wr32(dst + pos, cr[i].dst_len, big);
            memcpy(dst + pos + 4, tmp.data() + i * slot, cr[i].dst_len);
            pos += 4 + cr[i].dst_len;
            while (pos & 127) dst[pos++] = 0;
        }
        *dst_len = pos; return ALZ_OK;
    }
    }
    return ALZ_E_INVALID;
}
