// alz_measure.h -- decoded sizes without decoding: the launcher of the measure kernels (alz_measure.hip) for the host TU.
// Not part of the ABI (include/auroralz.h: alz_measure_batch / alz_measure_batch_device / alz_container_measure).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

// enqueue the measure kernel of one format over `count` streams (index list selects them; NULL = 0..count-1): results[i] becomes what
// alz_launch_decode would leave there for the same stream -- status, dst_len, src_used -- with dst_cap as a bound on the count only.
// Nothing but `d_results` is written.  `exact`: the counting sink under the exact parsers alone (alz_ctx_set_exact_kernels); otherwise
// the formats of alz_measure_has_bulk take the lane-parallel parse rounds for the bulk of a stream.
hipError_t alz_launch_measure(int fmt, hipStream_t stream, const void* d_src, const alz_stream* d_streams, const uint32_t* d_index,
                              uint32_t count, alz_result* d_results, const alz_lz_properties* lz, bool exact = false);
bool alz_measure_has_bulk(int fmt);

// ---- host side: the helper of alz_container.cpp that alz_container_measure.cpp shares (PRS.GetByteOrder: 1 little, 2 big, 0 none; the LZ4 / Snappy framing
// and its XXH32, which both files read, are alz_framing.h)
int alz_host_prs_byte_order(const uint8_t* src, size_t len);
