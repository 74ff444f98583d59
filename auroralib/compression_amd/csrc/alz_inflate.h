// alz_inflate.h -- DEFLATE (RFC 1951) as zlib's inflate implements it: the launchers of alz_inflate.hip for the host TU.
// Not part of the ABI (include/auroralz.h: alz_inflate_decode_batch / alz_inflate_measure_batch and their _device forms).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#define ALZ_INFLATE_WINDOW 0x8000u   /* the largest distance a distance symbol can name (symbol 29, 13 extra bits: 24577 + 8191) */

// enqueue the decode kernel over `count` streams (index list selects them; NULL = 0..count-1).  There is ONE decode kernel: every context
// mode runs it.
hipError_t alz_launch_inflate_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                     const uint32_t* d_index, uint32_t count, alz_result* d_results);
// the same parser on a counting sink: writes nothing but the results
hipError_t alz_launch_inflate_measure(hipStream_t stream, const void* d_src, const alz_stream* d_streams,
                                      const uint32_t* d_index, uint32_t count, alz_result* d_results);
