"""-m gpu: the LZ4 frame / legacy and Snappy file decode (csrc/alz_container.cpp: the host walk that turns a file into GPU work) against the
oracle's in-order reader, on generated files whose expected output comes from a byte-wise model (tests/framing_cases.py) and on seeded
structural mutations of them, at ample, exact, one-short, zero and mid-block capacities.  ALZ_FUZZ_SEED picks the files."""
import ctypes as C
import struct

import numpy as np
import pytest

import framing_cases as FC
import oracle_lib as O
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from auroralib.compression_amd._lib import AlzError, load

pytestmark = pytest.mark.gpu
CT = {"lz4": A.C_LZ4_FRAME, "legacy": A.C_LZ4_LEGACY, "snappy": A.C_SNAPPY}
CANARY = 0xA5
CASES = FC.generated_cases(O.xxh32)
COUNTERS = ("batch blocks", "split plan pairs", "tight-capacity retries", "fallback blocks", "linked blocks", "stored blocks")


def lib_decode(container, data, cap):
    """alz_container_decompress into a canary-filled host buffer of exactly `cap` bytes: (rc, status, dst_len, src_used, buffer)."""
    lib = load()
    lib.alz_container_decompress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    buf = np.full(max(cap, 1), CANARY, dtype=np.uint8)
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    o = A.ContainerOptions()
    rc = lib.alz_container_decompress(F._context().h, container, C.byref(o), data, len(data), buf.ctypes.data_as(C.c_void_p), cap, C.byref(dl), C.byref(su), C.byref(st))
    return rc, st.value, dl.value, su.value, buf


def oracle_decode(container, data, cap):
    dst = C.create_string_buffer(max(cap, 1))
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = O.lib.oracle_container_decompress(container, C.byref(O._opt(True, None)), data, len(data), dst, cap, C.byref(dl), C.byref(su), C.byref(st))
    return rc, st.value, dl.value, su.value, dst.raw[:dl.value]


def compare(case, cap):
    """Library against oracle at one capacity; returns a description of the first difference, or None."""
    ct = CT[case.container]
    g = lib_decode(ct, case.data, cap)
    o = oracle_decode(ct, case.data, cap)
    where = "%r cap=%d" % (case, cap)
    if case.container == "snappy" and g[0] == A.E_FORMAT and o[0] != A.E_FORMAT and FC.snappy_refusal_reached(case.data, cap):
        return None
    if g[0] != o[0]:
        return "%s: rc %d, oracle %d (status %d / %d)" % (where, g[0], o[0], g[1], o[1])
    if g[0] not in (0, A.E_STREAM):
        return None
    if (g[1], g[2]) != (o[1], o[2]):
        return "%s: status/dst_len %d/%d, oracle %d/%d" % (where, g[1], g[2], o[1], o[2])
    got = g[4][:g[2]].tobytes()
    if got != o[4]:
        i = next(k for k in range(len(got)) if got[k] != o[4][k])
        return "%s: first differing byte %d (%#x, oracle %#x)" % (where, i, got[i], o[4][i])
    if g[1] == A.ST_OK:
        if g[3] != o[3]:
            return "%s: src_used %d, oracle %d" % (where, g[3], o[3])
        tail = g[4][g[2]:cap]
        if tail.size and not (tail == CANARY).all():
            return "%s: byte %d past dst_len overwritten" % (where, g[2] + int(np.argmax(tail != CANARY)))
    return None


def capacities(case, rng, n):
    """ample, exact, one short, zero, and cut in the middle of a block"""
    j = rng.randrange(len(case.mids)) if case.mids else 0
    start, end = (case.mids[j], case.mids[j + 1] if j + 1 < len(case.mids) else n) if case.mids else (0, n)
    return sorted({n + 4096, n, max(n - 1, 0), 0, min(start + max(1, (end - start) // 2), n)})


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.label for c in CASES])
def test_generated_case_against_oracle_and_model(i):
    case = CASES[i]
    rng = FC.random.Random(case.seed)
    n = len(case.expect)
    rc, st, dl, su, buf = lib_decode(CT[case.container], case.data, n + 4096)
    assert (rc, st) == (0, A.ST_OK) and buf[:dl].tobytes() == case.expect, "%r: rc %d status %d, %d of %d bytes" % (case, rc, st, dl, n)
    bad = [e for cap in capacities(case, rng, n) for e in [compare(case, cap)] if e]
    assert not bad, bad[:5]


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.label for c in CASES])
def test_mutated_case_against_oracle(i):
    case = CASES[i]
    rng = FC.random.Random(FC.SEED * 7919 + i)
    bad = []
    for mu in FC.mutants(case, FC.SEED * 7919 + i):
        o = oracle_decode(CT[mu.container], mu.data, len(case.expect) + (1 << 20))
        n = o[2]
        for cap in sorted({len(case.expect) + (1 << 20), n, max(n - 1, 0), 0, rng.randrange(n + 1)}):
            e = compare(mu, cap)
            if e:
                bad.append(e)
    assert not bad, bad[:5]


# ------------------------------------------------------------------------------------------------ named regressions


def _frame(blocks, flg=0x40, bd=4, raw=None):
    return FC.lz4_frame(blocks, O.xxh32, flg=flg, bd=bd << 4, raw_flags=raw)


def test_offset0_match_in_a_linked_frame_reads_the_earlier_block():
    """Block 1 starts with an offset-0 match (distance 65 536, E1) after a 64 KiB block: it reads block 0's first bytes.  The independence walk did not
    count offset 0 as reaching back, so the block went into the batch with no history."""
    rng = FC.random.Random(3)
    b0 = rng.randbytes(0x10000)
    b1 = FC.lz4_seq(b"", 0, 20) + FC.lz4_seq(b"tail!")
    frame = _frame([b0, b1], raw=[True, False])
    expect = b0 + b0[:20] + b"tail!"
    assert O.container_decompress(A.C_LZ4_FRAME, frame, cap=len(expect)) == (expect, A.ST_OK)
    assert lib_decode(A.C_LZ4_FRAME, frame, len(expect))[4].tobytes() == expect
    assert F.LZ4().Decompress(frame) == expect


def test_block_checksum_fault_behind_a_truncated_block():
    """Block 1 is truncated inside its sequences, block 2 has a bad checksum (or a size above the block maximum): the in-order reader stops at block 1
    (EndOfStreamException); the checksum or size of block 2 was checked before anything was decoded."""
    rng = FC.random.Random(4)
    b0 = FC.lz4_seq(rng.randbytes(100))
    b1 = bytes([0xF0, 200]) + rng.randbytes(50)                                 # a 215-byte literal run with 50 bytes behind it
    b2 = FC.lz4_seq(rng.randbytes(30))
    frame = bytearray(_frame([b0, b1, b2], flg=0x40 | 16))
    frame[-5] ^= 1                                                              # block 2's checksum
    for data in (bytes(frame), bytes(frame[:-(4 + len(b2) + 4 + 4)]) + struct.pack("<I", 0x10001) + bytes(8)):
        o = oracle_decode(A.C_LZ4_FRAME, data, 4096)
        assert (o[0], o[1]) == (A.E_STREAM, A.ST_INPUT_TRUNCATED)
        assert compare(FC.Case("truncated block before a checksum / size fault", "lz4", data, None, [], 4), 4096) is None
        with pytest.raises(F.EndOfStreamException):
            F.LZ4().Decompress(data)
    # the same fault behind blocks that decode cleanly still decides
    good = bytearray(_frame([b0, b2, b2], flg=0x40 | 16)); good[-5] ^= 1
    assert lib_decode(A.C_LZ4_FRAME, bytes(good), 4096)[0] == oracle_decode(A.C_LZ4_FRAME, bytes(good), 4096)[0] == A.E_CHECKSUM


def test_snappy_stored_chunk_over_capacity_before_a_refused_chunk():
    """A stored chunk that overflows the capacity, then a compressed chunk of declared size 0 whose length runs past its varint: the in-order reader
    fails at the stored chunk (OUTPUT_CAPACITY); the refusal of the later chunk (E_FORMAT) was applied first."""
    raw = bytes(range(256)) * 8
    data = bytes([0xff, 6, 0, 0]) + b"sNaPpY" + bytes([1]) + (len(raw) + 4).to_bytes(3, "little") + bytes(4) + raw
    data += bytes([0, 7, 0, 0]) + bytes(4) + bytes([0, 0, 0])                  # varint 0, then two bytes the declared length still covers
    for cap in (1000, 0):
        o = oracle_decode(A.C_SNAPPY, data, cap)
        g = lib_decode(A.C_SNAPPY, data, cap)
        assert (o[0], o[1], o[2]) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, 0)
        assert (g[0], g[1], g[2]) == (o[0], o[1], o[2])
    with pytest.raises(BufferError):
        F.Snappy().Decompress(data, capacity=1000)
    assert lib_decode(A.C_SNAPPY, data, 4096)[0] == A.E_FORMAT                  # reached in file order: the documented refusal


def test_snappy_reserved_chunk_behind_a_stored_chunk_over_capacity():
    """The same order for a reserved (unskippable) chunk type: it was refused while the chunks were collected, before the stored chunk in front of it
    failed on the capacity."""
    raw = bytes(range(256)) * 8
    data = bytes([0xff, 6, 0, 0]) + b"sNaPpY" + bytes([1]) + (len(raw) + 4).to_bytes(3, "little") + bytes(4) + raw + bytes([0x02, 1, 0, 0, 0])
    o, g = oracle_decode(A.C_SNAPPY, data, 1000), lib_decode(A.C_SNAPPY, data, 1000)
    assert (o[0], o[1], o[2]) == (A.E_STREAM, A.ST_OUTPUT_CAPACITY, 0) and (g[0], g[1], g[2]) == (o[0], o[1], o[2])
    assert lib_decode(A.C_SNAPPY, data, 4096)[0] == oracle_decode(A.C_SNAPPY, data, 4096)[0] == A.E_FORMAT


def test_snappy_chunk_that_decodes_past_its_declared_size():
    """The managed decoder runs a chunk's elements while it has produced less than the declared size, so the last element may run past it, and the
    chunks behind it move.  Each chunk used to be cut at its declared size (OUTPUT_CAPACITY at any capacity: the format class grew its buffer to 2 GiB)."""
    body = bytes([4, 9 << 2]) + b"0123456789"                                      # declares 4 bytes, holds a 10-byte literal
    chunk = bytes([0, len(body) + 4, 0, 0]) + bytes(4) + body
    data = bytes([0xff, 6, 0, 0]) + b"sNaPpY" + chunk + bytes([1, 7, 0, 0]) + bytes(4) + b"abc" + chunk
    expect = b"0123456789abc0123456789"
    for cap in (len(expect), len(expect) + 100, 12, 5, 0):
        o = oracle_decode(A.C_SNAPPY, data, cap)
        assert o[4] == expect[:o[2]] and (o[1] == A.ST_OK) == (cap >= len(expect))
        assert compare(FC.Case("snappy chunk past its declared size", "snappy", data, None, [], 0), cap) is None, cap
    assert F.Snappy().Decompress(data) == expect


def test_stored_block_cut_at_the_capacity():
    """A stored block that does not fit writes what fits (the window clips it), as a compressed block does: dst_len is the capacity."""
    rng = FC.random.Random(5)
    b0, b1 = FC.lz4_seq(rng.randbytes(1000)), rng.randbytes(3000)
    for flg in (0x40, 0x60):
        frame = _frame([b0, b1, b0], flg=flg, raw=[False, True, False])
        for cap in (2500, 1000, 999, 4000, 3999):
            o = oracle_decode(A.C_LZ4_FRAME, frame, cap)
            assert (o[1], o[2]) == (A.ST_OUTPUT_CAPACITY, cap)
            assert compare(FC.Case("stored block at the capacity", "lz4", frame, None, [], 5), cap) is None, cap


def test_many_tiny_blocks_through_the_format_class():
    """20 000 one-byte blocks at BD 7: the capacity hint used to ask for 4 MiB per block (78 GiB), and the failed allocation escaped Decompress."""
    case = FC.many_tiny_blocks(O.xxh32)
    assert F._lz4_capacity_hint(case.data) <= 255 * len(case.data) + (1 << 16)
    assert F.LZ4().Decompress(case.data) == case.expect
    assert compare(case, len(case.expect)) is None


# ------------------------------------------------------------------------------------------------ format classes, branch counters


def _expected_exception(container, data):
    rc, st, _, _, out = oracle_decode(CT[container], data, 255 * len(data) + (1 << 16))     # (no file decodes to more)
    if rc == 0:
        return None, out
    if rc == A.E_FORMAT:
        return F.InvalidIdentifierException, None
    if rc == A.E_CHECKSUM:
        return F.InvalidDataException, None
    if rc == A.E_STREAM:
        return {A.ST_INPUT_TRUNCATED: F.EndOfStreamException, A.ST_OUTPUT_SIZE_MISMATCH: F.DecompressedSizeException,
                A.ST_OUTPUT_CAPACITY: BufferError}.get(st, ValueError), None
    return AlzError, None


def test_format_classes_on_a_subset():
    """F.LZ4 / F.LZ4Legacy / F.Snappy .Decompress(data) with no capacity: the model's bytes, or the exception the oracle's outcome maps to."""
    cls = {"lz4": F.LZ4, "legacy": F.LZ4Legacy, "snappy": F.Snappy}
    rng = FC.random.Random(FC.SEED)
    subset = [c for c in CASES if len(c.expect) < (8 << 20)]
    subset = rng.sample(subset, min(12, len(subset))) + [c for c in CASES if "larger than" in c.label]
    for case in subset:
        assert cls[case.container]().Decompress(case.data) == case.expect, case
        for mu in FC.mutants(case, rng.randrange(1 << 30), per_case=4):
            if mu.container == "snappy" and FC.snappy_refusal_reached(mu.data, 255 * len(mu.data) + (1 << 16)):
                continue
            exc, out = _expected_exception(mu.container, mu.data)
            if exc is None:
                assert cls[mu.container]().Decompress(mu.data) == out, mu
            else:
                with pytest.raises(exc):
                    cls[mu.container]().Decompress(mu.data)


def counters():
    lib = load()
    lib.alz_debug_container_counters.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    v = (C.c_uint64 * len(COUNTERS))()
    assert lib.alz_debug_container_counters(v, len(COUNTERS)) == len(COUNTERS)
    return list(v)


def test_every_branch_of_the_lz4_file_decode_runs():
    """The generated files reach every branch of the LZ4 file decode: the independent batch, the split (long + short) plans, the tight-capacity
    retry, in-order decoding after a fallback, linked frames and stored blocks -- counted by the library itself."""
    before = counters()
    for case in CASES:
        if case.container != "snappy":
            rc, st, dl, _, buf = lib_decode(CT[case.container], case.data, len(case.expect) + 4096)
            assert (rc, st, dl) == (0, A.ST_OK, len(case.expect)) and buf[:dl].tobytes() == case.expect, case
    moved = [a - b for a, b in zip(counters(), before)]
    assert all(moved), dict(zip(COUNTERS, moved))
