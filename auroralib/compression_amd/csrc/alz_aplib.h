// alz_aplib.h -- aPLib (Formats/Common/aPLib.cs), the last LzWindows user of the reference: the launchers of alz_aplib.hip for the host TU.
// Not part of the ABI (include/auroralz.h: alz_aplib_decode_batch / alz_aplib_measure_batch and their _device forms).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#define ALZ_APLIB_WINDOW 0x200000u   /* lzProperties[^1] = LzProperties(0x200000, ...): WindowsBits 21  aPLib.cs:35, :111 */

// enqueue the decode kernel over `count` streams (index list selects them; NULL = 0..count-1).  `family`: ALZ_APLIB_EXACT = DirectSink, one
// token at a time (alz_ctx_set_exact_kernels); ALZ_APLIB_PRODUCTION = the token-queue kernel (alz_ctx_set_kernel_variant != 0);
// ALZ_APLIB_DEFAULT = whichever of the two was measured faster (alz_aplib.hip: ALZ_APLIB_DEFAULT_IS_PRODUCTION).
enum { ALZ_APLIB_DEFAULT = 0, ALZ_APLIB_EXACT = 1, ALZ_APLIB_PRODUCTION = 2 };
hipError_t alz_launch_aplib_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                   const uint32_t* d_index, uint32_t count, alz_result* d_results, int family);
// the same parser on a counting sink: writes nothing but the results (one kernel serves both families)
hipError_t alz_launch_aplib_measure(hipStream_t stream, const void* d_src, const alz_stream* d_streams,
                                    const uint32_t* d_index, uint32_t count, alz_result* d_results);
