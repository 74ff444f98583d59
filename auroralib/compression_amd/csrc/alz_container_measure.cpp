// alz_container_measure.cpp -- alz_container_measure: the decompressed size of a file of a container WITHOUT a size field (PRS, LZO, FastLZ, LZ4 frame /
// legacy, framed Snappy) from its bodies measured on the GPU (alz_measure_batch).  The framing of the LZ4 and Snappy files is read by alz_framing.h, the
// same code alz_container.cpp's decoders read it with, and what the measured sizes make of a file is decided there too (lz4_replay,
// snappy_measure_replay): here the bodies are sent out.  This file is a translation unit of its own because it calls into the batch half of the
// library, which the header parsers of alz_container.cpp are built without (their sanitized fuzz binary).
#include <cstdint>
#include <vector>

#include "alz_framing.h"
#include "alz_measure.h"
#include "auroralz.h"

namespace {

using namespace alz_framing;

// ---------------------------------------------------------------------------------------------- sizes without decoding (alz_container_measure)
// A body measured with no bound on its count tells what it does in ANY destination (place_body, alz_framing.h).  So the bodies of a file go out as
// ONE batch, and the in-order reader is replayed over the results on the host.
inline alz_stream measured_body(uint32_t fmt, size_t off, size_t n) { return body(fmt, off, n, 0, kNoBound, 0); }

int measure(alz_ctx* ctx, const uint8_t* src, size_t len, std::vector<alz_stream>& ss, std::vector<alz_result>& rs) {
    rs.resize(ss.size());
    return ss.empty() ? ALZ_OK : alz_measure_batch(ctx, nullptr, (uint32_t)ss.size(), src, len, ss.data(), rs.data());
}

// LZ4.Decompress  Formats/Common/LZ4.cs:50-93 as the in-order reader sees the file, over measured block sizes: the frames are read once, their
// compressed blocks go out as ONE measure batch, and the reader is replayed over the results.  The content checksum is taken as correct.
int lz4_file_measure(alz_ctx* ctx, const uint8_t* src, size_t len, size_t cap, size_t* size_out, size_t* src_used, int32_t* status) {
    Lz4File w; std::vector<alz_stream> ss; std::vector<alz_result> rs;
    lz4_collect(src, len, w, [&](const Lz4Block& b) { ss.push_back(measured_body(ALZ_FMT_LZ4_BLOCK, b.off, b.len)); });
    if (const int e = measure(ctx, src, len, ss, rs)) return e;
    Lz4Sizes sizes;
    const Outcome o = lz4_replay(w, len, cap, rs.data(), sizes);
    if (size_out) *size_out = (size_t)o.out;
    if (src_used) *src_used = o.pos;
    if (status) *status = o.status;
    return o.rc;
}

// Snappy.Decompress  Formats/Common/Snappy.cs:39-69 over measured chunk sizes: collected at the declared places, measured as one batch, replayed; where
// the replay leaves the assumed positions the rest of the file is collected again from there.
int snappy_file_measure(alz_ctx* ctx, const uint8_t* src, size_t len, size_t cap, size_t* size_out, size_t* src_used, int32_t* status) {
    if (!snappy_has_id(src, len)) return ALZ_E_FORMAT;
    SnappyReader r = { 10, 0, 0 }; Outcome o;
    std::vector<alz_stream> ss; std::vector<alz_result> rs;
    do {
        ss.clear();
        snappy_measure_collect(src, len, r.pos, [&](size_t off) { ss.push_back(measured_body(ALZ_FMT_SNAPPY_RAW, off, len - off)); });
        if (const int e = measure(ctx, src, len, ss, rs)) return e;
    } while (!snappy_measure_replay(src, len, cap, r, 0, ss.data(), ss.size(), rs.data(), o));
    if (o.rc != ALZ_OK && o.rc != ALZ_E_STREAM) return o.rc;
    if (size_out) *size_out = (size_t)o.out;
    if (src_used) *src_used = o.pos;
    if (status) *status = o.status;
    return o.rc;
}

}  // namespace

extern "C" {

// Decompressed size of a file of a container without a size field, by measuring its bodies on the GPU (include/auroralz.h)
int alz_container_measure(alz_ctx* ctx, uint32_t container, const alz_container_options* opt, const uint8_t* src, size_t len, size_t size_limit,
                          size_t* size_out, size_t* src_used, int32_t* status) {
    (void)opt;
    if (!ctx || !src) return ALZ_E_INVALID;
    alz_stream ss[2]; alz_result rs[2]; uint32_t n = 1;
    switch (container) {
    case ALZ_C_PRS: {                                                                       // PRS.cs:42-57: the detected byte order, then the other one
        const bool first_big = alz_host_prs_byte_order(src, len) == 2;
        ss[0] = measured_body(first_big ? ALZ_FMT_PRS_BE : ALZ_FMT_PRS_LE, 0, len);
        ss[1] = measured_body(first_big ? ALZ_FMT_PRS_LE : ALZ_FMT_PRS_BE, 0, len);
        n = 2;
        break;
    }
    case ALZ_C_LZO: ss[0] = measured_body(ALZ_FMT_LZO, 0, len); break;                      // LZO.cs:42-43
    case ALZ_C_FASTLZ: ss[0] = measured_body(ALZ_FMT_FASTLZ, 0, len); break;                // FastLZ.cs:40-52
    case ALZ_C_LZ4_LEGACY: case ALZ_C_LZ4_FRAME: return lz4_file_measure(ctx, src, len, size_limit, size_out, src_used, status);
    case ALZ_C_SNAPPY: return snappy_file_measure(ctx, src, len, size_limit, size_out, src_used, status);
    default: return ALZ_E_UNSUPPORTED;
    }
    for (uint32_t i = 0; i < n; i++) ss[i].dst_cap = clamp32(size_limit);                   // (one body: the limit is its capacity, as run_body passes it)
    const int rc = alz_measure_batch(ctx, nullptr, n, src, len, ss, rs);
    if (rc != ALZ_OK) return rc;
    const alz_result& r = (n == 2 && rs[0].status != ALZ_ST_OK) ? rs[1] : rs[0];
    if (size_out) *size_out = r.dst_len;
    if (src_used) *src_used = r.src_used;
    if (status) *status = r.status;
    return r.status == ALZ_ST_OK ? ALZ_OK : ALZ_E_STREAM;
}

}  // extern "C"
