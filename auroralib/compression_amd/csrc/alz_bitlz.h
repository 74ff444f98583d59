// alz_bitlz.h -- CRILAYLA (CRI/CRILAYLA.cs) and ALLZ (Specialized/ALLZ.cs), the two bit-stream LZ bodies of the reference's .Extended
// assembly: the launcher of alz_bitlz.hip for the host TU.  Not part of the ABI (include/auroralz.h: alz_bitlz_decode_batch and its _device form).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#define ALZ_CRILAYLA_MAXDIST 8194u   /* 13-bit field + 3  CRILAYLA.cs:136 */
#define ALZ_CRILAYLA_HEADER 0x100u   /* the plain bytes a CRILAYLA file keeps behind its body  CRILAYLA.cs:18 */

// enqueue the kernel of `kind` (an alz_bitlz_kind) over `count` streams (index list selects them; NULL = 0..count-1).  Each format has ONE
// kernel -- the exact one, every token executed as it is parsed -- so all three context modes run it.
hipError_t alz_launch_bitlz_decode(int kind, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                   const uint32_t* d_index, uint32_t count, alz_result* d_results);
