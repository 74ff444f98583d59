// alz_rlh.h -- the two non-LZ members of the Nintendo GBA / DS family (RLE30, HUF20): the launchers of alz_rlh.hip for the host TU.
// Not part of the ABI (include/auroralz.h: alz_rlh_decode_batch / alz_rlh_encode_batch, alz_rlhudson_decode_batch / alz_rlhudson_encode_batch
// and their _device forms).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

// enqueue the decode kernel of one alz_rlh_format over `count` streams (index list selects them; NULL = 0..count-1).
// `exact`: one token / one bit at a time (alz_ctx_set_exact_kernels); otherwise the lane-parallel kernel where the format has one.
hipError_t alz_launch_rlh_decode(int fmt, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                 const uint32_t* d_index, uint32_t count, alz_result* d_results, bool exact);
// the same for RLE30.CompressHeaderless (ALZ_RLH_RLE30 only: HUF20 has no encoder, include/auroralz.h says why)
hipError_t alz_launch_rlh_encode(int fmt, hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                 const uint32_t* d_index, uint32_t count, alz_result* d_results, bool exact);
bool alz_rlh_has_production(int fmt, bool encode);   // is there a lane-parallel kernel beside the exact one
// RLHudson (alz_rlhudson_*), RLE30's sibling outside alz_rlh_format: the same two decode kernels and the one encode kernel over its own grammar
hipError_t alz_launch_rlhudson_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                      const uint32_t* d_index, uint32_t count, alz_result* d_results, bool exact);
hipError_t alz_launch_rlhudson_encode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                      const uint32_t* d_index, uint32_t count, alz_result* d_results);
