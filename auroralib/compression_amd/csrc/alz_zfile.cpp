// alz_zfile.cpp -- ZLib and GZip files in batches: alz_zfile_decode_batch / alz_zfile_measure_batch.  What alz_zlib_decompress /
// alz_gzip_decompress (alz_inflate_file.cpp) do for one file, for a whole set in one call: the header walks on the host (alz_zfile.h, the
// code of the single-file layer), the source uploaded once, all bodies as ONE alz_inflate_decode_batch_device (or measure batch), all outputs
// summed in HBM by alz_checksum_batch_device (Adler-32 for the ZLib files, CRC-32 for the GZip members), the trailers compared on the host,
// the outputs downloaded once.  A GZip member behind the first is found only when the one before it is decoded, so the batch runs in
// rounds: round r holds the r-th member of every file that has one.  Pure host code on the public ABI.
#include <algorithm>
#include <cstring>
#include <vector>

#include "auroralz.h"
#include "alz_file_batch.h"
#include "alz_zfile.h"

namespace {

using namespace alz_zframe;
using namespace alz_file_batch;

struct FileState { size_t pos = 0, out = 0; bool active = false; };            // where the next body starts, bytes delivered so far

int finish(alz_file_result& r, FileState& f, int rc, int32_t status, size_t out, size_t used) {
    r.rc = rc; r.status = status; r.dst_len = (uint32_t)out; r.src_used = (uint32_t)used;
    f.active = false;
    return rc;
}

// the header of file i's next member (of the ZLib file: its only one); the file stays active when a body follows
void open_member(const alz_stream& file, const uint8_t* src, FileState& f, alz_file_result& r) {
    const size_t len = file.src_len;
    if (file.format == ALZ_ZFILE_ZLIB) {
        if (int rc = zlib_header(src, len)) { finish(r, f, rc, ALZ_ST_OK, 0, 0); return; }
        f.pos = kZlibHeader;
    } else {
        const int hrc = gzip_header(src, len, f.pos);
        if (hrc == ALZ_E_STREAM) { finish(r, f, ALZ_E_STREAM, ALZ_ST_INPUT_TRUNCATED, f.out, len); return; }
        if (hrc) { finish(r, f, hrc, ALZ_ST_OK, f.out, f.pos); return; }
    }
    f.active = true;
}

// what the body of file i's member returned, its trailer against `sum` (NULL: a measure, the checksum is taken as correct), the next member
void close_member(const alz_stream& file, const uint8_t* src, FileState& f, alz_file_result& r, const alz_result& b, const uint32_t* sum) {
    const size_t len = file.src_len;
    if (file.format == ALZ_ZFILE_ZLIB) {
        if (b.status != ALZ_ST_OK) { finish(r, f, ALZ_E_STREAM, b.status, b.dst_len, kZlibHeader + (size_t)b.src_used); return; }
        const size_t pos = kZlibHeader + (size_t)b.src_used;
        if (len - pos < kZlibTrailer) { finish(r, f, ALZ_E_STREAM, ALZ_ST_INPUT_TRUNCATED, b.dst_len, len); return; }
        finish(r, f, sum && !zlib_trailer_ok(src + pos, *sum) ? ALZ_E_CHECKSUM : ALZ_OK, ALZ_ST_OK, b.dst_len, pos + kZlibTrailer);
        return;
    }
    f.out += b.dst_len;
    if (b.status != ALZ_ST_OK) { finish(r, f, ALZ_E_STREAM, b.status, f.out, f.pos + (size_t)b.src_used); return; }
    f.pos += (size_t)b.src_used;
    if (len - f.pos < kGzipTrailer) { finish(r, f, ALZ_E_STREAM, ALZ_ST_INPUT_TRUNCATED, f.out, len); return; }
    if (!gzip_trailer_ok(src + f.pos, sum, b.dst_len)) { finish(r, f, ALZ_E_CHECKSUM, ALZ_ST_OK, f.out, f.pos + kGzipTrailer); return; }
    f.pos += kGzipTrailer;
    if (!gzip_member_follows(src, len, f.pos)) { finish(r, f, ALZ_OK, ALZ_ST_OK, f.out, len); return; }   // source.Position = source.Length  GZip.cs:33
    open_member(file, src, f, r);
}

int run(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files, uint8_t* dst_base, size_t dst_bytes,
        alz_file_result* results, bool measure) {
    if (int rc = check_files(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, !measure, [](uint32_t format) { return format <= ALZ_ZFILE_GZIP; })) return rc;
    if (n == 0) return ALZ_OK;
    std::vector<FileState> state(n);
    uint32_t active = 0;
    for (uint32_t i = 0; i < n; i++) {
        results[i] = alz_file_result{ALZ_OK, ALZ_ST_OK, 0, 0};
        open_member(files[i], src_base + files[i].src_off, state[i], results[i]);
        active += state[i].active;
    }
    if (!active) return ALZ_OK;                                                 // every file ended in its header: nothing for the GPU

    DeviceBuffer d_src(ctx), d_dst(ctx);
    int rc;
    if ((rc = d_src.alloc(src_bytes)) || (rc = alz_memcpy_h2d(ctx, d_src.p, src_base, src_bytes))) return rc;
    if (!measure && (rc = d_dst.alloc(dst_bytes))) return rc;

    std::vector<uint32_t> who;                                                  // the files of this round
    std::vector<alz_stream> bodies, ranges[2];
    std::vector<alz_result> got;
    std::vector<uint32_t> sums[2], slot;
    while (active) {
        who.clear(); bodies.clear();
        for (uint32_t i = 0; i < n; i++) {
            if (!state[i].active) continue;
            const size_t room = (size_t)files[i].dst_cap - state[i].out;
            alz_stream s; memset(&s, 0, sizeof(s));
            s.src_off = files[i].src_off + state[i].pos;
            s.src_len = (uint32_t)(files[i].src_len - state[i].pos);
            s.dst_off = files[i].dst_off + state[i].out;
            s.dst_cap = room > kMaxCap ? kMaxCap : (uint32_t)room;
            who.push_back(i); bodies.push_back(s);
        }
        const uint32_t m = (uint32_t)who.size();
        got.assign(m, alz_result{0, 0, 0, 0});
        rc = measure ? alz_inflate_measure_batch_device(ctx, m, (const uint8_t*)d_src.p, src_bytes, bodies.data(), got.data())
                     : alz_inflate_decode_batch_device(ctx, m, (const uint8_t*)d_src.p, src_bytes, bodies.data(), (uint8_t*)d_dst.p, dst_bytes, got.data());
        if (rc) return rc;
        slot.assign(m, 0);
        if (!measure) {                                                         // the outputs that will meet a trailer, summed where they lie
            for (int k = 0; k < 2; k++) ranges[k].clear();
            for (uint32_t j = 0; j < m; j++) {
                if (got[j].status != ALZ_ST_OK) continue;
                const uint32_t kind = files[who[j]].format == ALZ_ZFILE_ZLIB ? ALZ_CK_ADLER32 : ALZ_CK_CRC32;
                alz_stream s; memset(&s, 0, sizeof(s));
                s.src_off = bodies[j].dst_off; s.src_len = got[j].dst_len;
                slot[j] = (uint32_t)ranges[kind].size();
                ranges[kind].push_back(s);
            }
            for (uint32_t kind = 0; kind < 2; kind++) {
                sums[kind].assign(ranges[kind].size(), 0);
                if (ranges[kind].empty()) continue;
                if ((rc = alz_checksum_batch_device(ctx, kind, (uint32_t)ranges[kind].size(), (const uint8_t*)d_dst.p, dst_bytes, ranges[kind].data(), sums[kind].data()))) return rc;
            }
        }
        for (uint32_t j = 0; j < m; j++) {
            const uint32_t i = who[j];
            const uint32_t kind = files[i].format == ALZ_ZFILE_ZLIB ? ALZ_CK_ADLER32 : ALZ_CK_CRC32;
            const uint32_t* sum = !measure && got[j].status == ALZ_ST_OK ? &sums[kind][slot[j]] : nullptr;
            close_member(files[i], src_base + files[i].src_off, state[i], results[i], got[j], sum);
            if (!state[i].active) active--;
        }
    }
    return measure ? ALZ_OK : download(ctx, n, files, results, d_dst.p, dst_base);
}

}   // namespace

int alz_zfile_decode_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                           uint8_t* dst_base, size_t dst_bytes, alz_file_result* results) {
    return run(ctx, n, src_base, src_bytes, files, dst_base, dst_bytes, results, false);
}
int alz_zfile_measure_batch(alz_ctx* ctx, uint32_t n, const uint8_t* src_base, size_t src_bytes, const alz_stream* files,
                            alz_file_result* results) {
    return run(ctx, n, src_base, src_bytes, files, nullptr, 0, results, true);
}
