// alz_file_batch.h -- what the batched file layers (alz_zfile.cpp: ZLib / GZip; alz_framed_batch.cpp: LZ4 / Snappy) share: a device buffer
// that is freed on every exit path, the range test of their argument checks, and the one download of all outputs.  Pure host code on the
// public ABI; not part of it.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "auroralz.h"

namespace alz_file_batch {

struct DeviceBuffer {                                                           // freed on every exit path
    alz_ctx* ctx; void* p = nullptr;
    explicit DeviceBuffer(alz_ctx* c) : ctx(c) {}
    ~DeviceBuffer() { if (p) (void)alz_device_free(ctx, p); }
    int alloc(size_t bytes) { return alz_device_malloc(ctx, bytes ? bytes : 1, &p); }
};

inline bool range_ok(uint64_t off, uint64_t len, uint64_t total) { return off <= total && len <= total - off; }

// the produced bytes of every file, device -> host: neighbouring outputs travel as one copy (through a bounce buffer, so that nothing
// between two outputs is written on the host)
inline int download(alz_ctx* ctx, uint32_t n, const alz_stream* files, const alz_file_result* results, const void* d_dst, uint8_t* dst) {
    const size_t kGap = 64u << 10, kPiece = 64u << 20;
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < n; i++) if (results[i].dst_len) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return files[a].dst_off < files[b].dst_off; });
    std::vector<uint8_t> bounce;
    for (size_t k = 0; k < order.size();) {
        const uint64_t lo = files[order[k]].dst_off;
        uint64_t hi = lo + results[order[k]].dst_len;
        size_t e = k + 1;
        for (; e < order.size(); e++) {
            const uint64_t a = files[order[e]].dst_off, b = a + results[order[e]].dst_len;
            if (a > hi + kGap || (b > hi ? b : hi) - lo > kPiece) break;
            if (b > hi) hi = b;
        }
        if (e == k + 1) {                                                       // a lone output goes straight to its place
            if (int rc = alz_memcpy_d2h(ctx, dst + lo, (const uint8_t*)d_dst + lo, (size_t)(hi - lo))) return rc;
        } else {
            bounce.resize((size_t)(hi - lo));
            if (int rc = alz_memcpy_d2h(ctx, bounce.data(), (const uint8_t*)d_dst + lo, bounce.size())) return rc;
            for (size_t j = k; j < e; j++)
                memcpy(dst + files[order[j]].dst_off, bounce.data() + (files[order[j]].dst_off - lo), results[order[j]].dst_len);
        }
        k = e;
    }
    return ALZ_OK;
}

}   // namespace alz_file_batch
