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

// ---- the same two bodies WRITTEN (alz_encode.hip; include/auroralz.h: alz_bitenc_*).  Encoder formats behind the public enum: the slots of an encode
// batch are 0 .. ALZ_FMT_COUNT - 1 the public formats, ALZ_FMT_COUNT FastLZ level 2, then these.  alz_encode_batch* never lets a caller name one;
// alz_bitenc_encode_batch* translates its alz_bitlz_kind into them.  (Here and not in alz_internal.h: the decoder's committed counters are hashed over that file.)
enum { ALZ_ENCFMT_CRILAYLA = ALZ_FMT_COUNT + 1, ALZ_ENCFMT_ALLZ = ALZ_FMT_COUNT + 2, ALZ_ENCFMT_COUNT = ALZ_FMT_COUNT + 3 };
// ... and aPLib's body (Formats/Common/aPLib.cs:183-286; include/auroralz.h: alz_apenc_*), the third one behind the enum.  ALZ_ENCFMT_END: what is sized by the number of slots
enum { ALZ_ENCFMT_APLIB = ALZ_FMT_COUNT + 3, ALZ_ENCFMT_END = ALZ_FMT_COUNT + 4 };
// d[i] = s[len - 1 - i] for the streams of d_index: s = d_src + d_orig_off[stream]; d is where d_streams[stream].src_off points (counted from
// d_src, as every descriptor's), a place inside the scratch d_rev with 64 readable bytes behind each copy  CRILAYLA.cs:204-206,253-257
hipError_t alz_launch_encode_reverse(hipStream_t stream, const void* d_src, void* d_rev, const alz_stream* d_streams, const uint64_t* d_orig_off,
                                     const uint32_t* d_index, uint32_t count, uint32_t max_len);
