// alz_xxh32.h -- XXH32 (the checksum of the LZ4 frame format) over byte ranges in HBM, and a range-copy kernel (HBM to HBM) for the stored
// blocks and chunks of the batched LZ4 / Snappy file layer: the launchers of alz_xxh32.hip for the host TU, and the host-side call of the
// copy for alz_framed_batch.cpp.  Not part of the ABI (include/auroralz.h: alz_xxh32_batch, alz_xxh32_batch_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#define ALZ_XXH32_UNROLL 4u          /* stripes of 16 bytes whose loads one loop iteration issues in front of its multiply chain */
#define ALZ_COPY_PIECE 16384u        /* bytes of a range one wavefront copies (a multiple of 16) */

// One range of a copy: n bytes from d_src + src_off to d_dst + dst_off.  `first`: the number of pieces in front of this range (filled in by
// alz_host_range_copy); a range of n bytes has ceil(n / ALZ_COPY_PIECE) pieces.
struct alz_copy_range { uint64_t src_off, dst_off; uint32_t n, first; };

// d_out[i] = XXH32 of range i (src_off / src_len of its alz_stream) with `seed`.  One launch; 4 lanes per range.
hipError_t alz_launch_xxh32(hipStream_t stream, uint32_t seed, const void* d_src, const alz_stream* d_ranges, uint32_t n, uint32_t* d_out);
// copies every range; `pieces` = all pieces of all ranges (> 0).  One launch; one wavefront per piece.  Writes nothing outside a range's
// [dst_off, dst_off + n); reads the source in aligned dwords that each hold a byte of the range.
hipError_t alz_launch_range_copy(hipStream_t stream, const void* d_src, void* d_dst, const alz_copy_range* d_ranges, uint32_t n, uint32_t pieces);

// The copy as a call on a context, for host code above the ABI: checks every range against src_bytes / dst_bytes (ALZ_E_INVALID), uploads
// the table, launches on the context's stream and waits.  `ranges[i].first` is overwritten.  n == 0, or no byte to copy, is ALZ_OK.
extern "C" int alz_host_range_copy(alz_ctx* ctx, uint32_t n, alz_copy_range* ranges, const uint8_t* d_src, size_t src_bytes, uint8_t* d_dst, size_t dst_bytes);
