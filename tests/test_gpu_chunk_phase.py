"""-m gpu: the built streams of tests/chunk_phase_cases.py through the token-queue decoders -- the chunked copy phase (csrc/alz_emit_chunk.h: the ring /
read-back line, alignment, far sources at the stream start, self-overlap, long tokens, dependency chains, the ring seam and its mirror, step composition,
literal runs, the capacity cut) and the element walk of the parse rounds (lane_walk_pos and the *_parse_round functions of csrc/alz_decode_fast.h: landing
offsets, element counts, refused elements, the input margin).  tests/test_chunk_phase_cpu.py pins every stream from the reference side.

One test per (row, family) that has streams (chunk_phase_cases.has_cases).  Every batch goes through test_gpu_scalar_paths.run -- the host ABI on both kernel families against the oracle, the expansion of
the token list against the result, canary-filled device buffers in kernel variants 1 and 2 (variant 2 is alz_decode_queue2_kernel for LZ4 / LZO / Snappy) --
and through test_gpu_measure.measure_parity (the bulk measure kernels share the parse rounds).  The PRS rows also run through the work queue of chunks."""
import pytest

import chunk_phase_cases as CP
import test_gpu_scalar_paths as SP
from auroralib.compression_amd import synth
from gpu_common import pack_streams
from test_chunk_phase_cpu import POPULATED, expanded
from test_gpu_measure import measure_parity

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row_name,family", POPULATED)
def test_built_streams(row_name, family):
    row = CP.ROWS[row_name]
    built = CP.cases(row_name, family)
    assert built, (row_name, family)
    items = []
    for (name, toks, ex), want in zip(built, expanded(row_name, family)):
        it = CP.item(row, toks, ex, want)
        it["what"] = name
        if ex.get("residues"):                           # C2: every destination residue 0 .. 15 (each stream shifts the ones behind it by one byte)
            items += [dict(it, dst_misalign=1) for _ in range(16)]
        else:
            items.append(it)
    what = "%s %s" % (row_name, family)
    streams, src, dst_bytes = pack_streams(items, dst_slack=16)
    if family == "C2":
        residues = [int(x) % 16 for x in synth.stream_records(streams)["dst_off"]]
        for k in range(0, len(items), 16):
            assert sorted(residues[k:k + 16]) == list(range(16)), (what, k)
    SP.run(items, what, lz=row.lz, queue=False)
    measure_parity(streams, src, dst_bytes, lz=row.lz, what=what + ", measured")
    if row_name.startswith("prs_"):
        SP.run(items, what + ", work queue", lz=row.lz, queue=True)
