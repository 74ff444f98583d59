"""-m gpu: decoded sizes without decoding (alz_measure_batch / alz_measure_batch_device / alz_container_measure) against the oracle.

The contract: for every stream, format and dst_cap the measure result equals the alz_result of a decode of the same alz_stream --
status and dst_len always, src_used wherever the header defines it (every status but OUTPUT_CAPACITY: the rule of gpu_common._check) --
on both tiers (the counting sink under the exact parsers alone / lane-parallel parse rounds for the bulk).  No tolerance anywhere."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import framing_cases as FC
import oracle_lib as O
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd import formats as F
from auroralib.compression_amd import synth
from auroralib.compression_amd.batch import Context, Plan, layout_from_results
from auroralib.compression_amd._lib import load
from gpu_common import ctx, pack_streams

pytestmark = pytest.mark.gpu
ALL = list(range(A.FMT_COUNT))
SIZELESS = (A.FMT_PRS_BE, A.FMT_LZ4_BLOCK, A.FMT_LZO, A.FMT_FASTLZ, A.FMT_SNAPPY_RAW)
NO_BOUND = 0xFFFFFF00
CT = {"lz4": A.C_LZ4_FRAME, "legacy": A.C_LZ4_LEGACY, "snappy": A.C_SNAPPY}
CASES = FC.generated_cases(O.xxh32)
CHECKSUM_ONLY_CASES = ("bd4 flags 44", "linked, in front of the second frame's start", "frame+skippable+legacy+frame+junk")


def clone(streams):
    out = (A.Stream * len(streams))()
    C.memmove(out, streams, C.sizeof(out))
    return out


def assert_same_results(g_res, o_res, what):
    gr, orr = synth.result_records(g_res), synth.result_records(o_res)
    bad = np.nonzero((gr["status"] != orr["status"]) | (gr["dst_len"] != orr["dst_len"]))[0]
    assert bad.size == 0, "%s: stream %d: measure(status=%d,len=%d) oracle(status=%d,len=%d)" % (
        what, bad[0], gr["status"][bad[0]], gr["dst_len"][bad[0]], orr["status"][bad[0]], orr["dst_len"][bad[0]])
    ok = orr["status"] != A.ST_OUTPUT_CAPACITY
    badu = np.nonzero(ok & (gr["src_used"] != orr["src_used"]))[0]
    assert badu.size == 0, "%s: stream %d src_used measure=%d oracle=%d" % (what, badu[0], gr["src_used"][badu[0]], orr["src_used"][badu[0]])


def measure_parity(streams, src, dst_bytes, lz=None, what=""):
    """measure_batch on both tiers against the oracle's decode of the same streams (their own dst_cap)."""
    _, o_res = O.decode_batch(streams, src, dst_bytes, lz=lz, nthreads=8)
    for exact in (1, 0):
        ctx().set_exact_kernels(exact)
        try:
            g_res = ctx().measure_batch(streams, src, lz=lz)
        finally:
            ctx().set_exact_kernels(0)
        assert_same_results(g_res, o_res, what + (" [exact tier]" if exact else " [bulk tier]"))
    return o_res


# ------------------------------------------------------------------------------------------------ 1. parity with the decoder's results


@pytest.mark.parametrize("fmt", ALL)
def test_parity_synthetic(fmt):
    sizes = np.array([1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 19, 31, 63, 64, 65, 100, 255, 256, 257, 1000, 1023, 1024, 1025,
                      4095, 4096, 4097, 5000, 8191, 8192, 8193, 10000], dtype=np.uint32)
    b = synth.make_batch(fmt, len(sizes), sizes, synth.seed_for(90 + fmt), dst_align=16)
    measure_parity(b.streams, b.src, b.dst_bytes, what=A.FORMAT_NAMES[fmt])
    for target, n in ((65536, 96), (262144, 24)):
        b = synth.make_batch(fmt, n, target, synth.seed_for(20 + fmt, target))
        o_res = measure_parity(b.streams, b.src, b.dst_bytes, what="%s %d" % (A.FORMAT_NAMES[fmt], target))
        orr = synth.result_records(o_res)
        assert (orr["status"] == 0).all() and (orr["dst_len"] == target).all()


def test_parity_mixed_format_batch():
    n = 256
    fm = np.array([[A.FMT_LZ10, A.FMT_LZ11, A.FMT_YAZ0, A.FMT_PRS_BE, A.FMT_LZ4_BLOCK, A.FMT_LZO, A.FMT_SNAPPY_RAW][i % 7] for i in range(n)], dtype=np.uint32)
    b = synth.make_batch(fm, n, 65536, synth.seed_for(4))
    measure_parity(b.streams, b.src, b.dst_bytes, what="mixed")


def test_parity_lzss_geometries():
    for bits in [(8, 4, 2), (10, 6, 2), (12, 4, 2), (13, 5, 2), (14, 4, 2), (16, 8, 2)]:
        lz = A.LzProperties.from_bits(*bits)
        b = synth.make_batch(A.FMT_LZSS, 16, np.array([300, 5000, 70000, 9] * 4, dtype=np.uint32), synth.seed_for(70, bits[0]), lz=lz)
        measure_parity(b.streams, b.src, b.dst_bytes, lz=lz, what="lzss%r" % (bits,))


def test_parity_handcrafted_edge_tokens():
    from cases import handcrafted_items
    streams, src, dst_bytes = pack_streams(handcrafted_items(), dst_slack=16)
    measure_parity(streams, src, dst_bytes, what="handcrafted")


def test_parity_unaligned_buffers():
    from cases import unaligned_items
    streams, src, dst_bytes = pack_streams(unaligned_items(), dst_slack=8)
    measure_parity(streams, src, dst_bytes, what="unaligned")


@pytest.mark.parametrize("fmt", ALL)
def test_parity_truncated_inputs(fmt, test_bmp):
    from cases import truncated_items
    streams, src, dst_bytes = pack_streams(truncated_items(fmt, test_bmp))
    measure_parity(streams, src, dst_bytes, what="trunc " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("fmt", ALL)
def test_parity_capacity_and_size_mismatch(fmt, test_bmp):
    from cases import capacity_items
    streams, src, dst_bytes = pack_streams(capacity_items(fmt, test_bmp), dst_slack=32)
    measure_parity(streams, src, dst_bytes, what="cap " + A.FORMAT_NAMES[fmt])


@pytest.mark.parametrize("fmt", ALL)
def test_parity_fuzz_garbage_and_mutations(fmt, test_bmp):
    from cases import fuzz_items
    streams, src, dst_bytes = pack_streams(fuzz_items(fmt, test_bmp, seed=FC.SEED), dst_slack=32)
    measure_parity(streams, src, dst_bytes, what="fuzz " + A.FORMAT_NAMES[fmt])


def test_parity_prs_terminator_inside_the_bulk_path(test_bmp):
    """PRS ends at its zero word wherever that is: with trailing data behind it the terminator is met by a parse round, not by the tail parser."""
    import os
    items = []
    for fmt in (A.FMT_PRS_BE, A.FMT_PRS_LE):
        for size, q in ((30000, 8), (5000, 0), (200, 4)):
            comp, _ = O.encode_stream(fmt, test_bmp[3000:3000 + size], quality=q)
            for tail in (os.urandom(3000), bytes(2000), comp):
                items.append(dict(fmt=fmt, src=comp + tail, decom_len=0, cap=size + 64))
    streams, src, dst_bytes = pack_streams(items)
    o_res = measure_parity(streams, src, dst_bytes, what="prs trailing data")
    assert (synth.result_records(o_res)["status"] == 0).all()


# ------------------------------------------------------------------------------------------------ 2. a large bound gives the true size


@pytest.mark.parametrize("fmt", ALL)
def test_large_bound_gives_the_true_size(fmt, test_bmp):
    sizes = np.array([1, 17, 300, 4097, 10000, 65536, 70001, 262144, 100001, 64], dtype=np.uint32)
    b = synth.make_batch(fmt, len(sizes), sizes, synth.seed_for(91 + fmt), dst_align=16)
    items = []
    for off, size, q in [(0, 10240, 8), (4096, 65536, 0), (100000, 262144, 8)]:
        comp, aux = O.encode_stream(fmt, test_bmp[off:off + size], quality=q)
        items.append(dict(fmt=fmt, src=comp, decom_len=size, aux0=aux.aux0, aux1=aux.aux1))
    for streams, src, dst_bytes in ((b.streams, b.src, b.dst_bytes), pack_streams(items)):
        _, o_res = O.decode_batch(streams, src, dst_bytes, nthreads=8)
        orr = synth.result_records(o_res)
        assert (orr["status"] == 0).all()
        wide = clone(streams)
        for s in wide:
            s.dst_off, s.dst_cap = 0, NO_BOUND
        for exact in (1, 0):
            ctx().set_exact_kernels(exact)
            try:
                gr = synth.result_records(ctx().measure_batch(wide, src))
            finally:
                ctx().set_exact_kernels(0)
            assert (gr["status"] == 0).all() and np.array_equal(gr["dst_len"], orr["dst_len"]) and np.array_equal(gr["src_used"], orr["src_used"]), (A.FORMAT_NAMES[fmt], exact)


# ------------------------------------------------------------------------------------------------ 3. nothing is written


def test_nothing_is_written_and_no_destination_is_needed():
    fm = np.array([ALL[i % len(ALL)] for i in range(200)], dtype=np.uint32)
    b = synth.make_batch(fm, len(fm), 20000, synth.seed_for(92))
    _, o_res = O.decode_batch(b.streams, b.src, b.dst_bytes, nthreads=8)
    canary_bytes = 1 << 20
    with Context(0) as c:                                       # a context of its own: nothing else has allocated on it
        d_src = c.malloc(b.src.nbytes)
        c.h2d(d_src, b.src)
        assert_same_results(c.measure_batch_device(b.streams, d_src, b.src.nbytes), o_res, "no destination allocated at all")
        d_can = c.malloc(canary_bytes)                          # stands where a destination would be: the next allocation of the context
        c.memset(d_can, 0xA5, canary_bytes)
        c.synchronize()
        for exact in (1, 0):
            c.set_exact_kernels(exact)
            assert_same_results(c.measure_batch_device(b.streams, d_src, b.src.nbytes), o_res, "device source, tier %d" % exact)
            assert c.last_kernel_ms() > 0
        assert (c.d2h(d_can, canary_bytes) == 0xA5).all()
        assert np.array_equal(c.d2h(d_src, b.src.nbytes), b.src)
        c.free(d_can)
        c.free(d_src)


# ------------------------------------------------------------------------------------------------ 4. two-pass decode


@pytest.mark.parametrize("fmt", SIZELESS)
def test_two_pass_decode_into_an_exactly_sized_buffer(fmt):
    rng = random.Random(93 + fmt)
    n = 300
    sizes = np.array([rng.choice([1, 100, 4096, 70000]) + rng.randrange(60000) for _ in range(n)], dtype=np.uint32)
    b = synth.make_batch(fmt, n, sizes, synth.seed_for(93 + fmt))
    o_dst, o_res = O.decode_batch(b.streams, b.src, b.dst_bytes, nthreads=8)
    orr, osr = synth.result_records(o_res), synth.stream_records(b.streams)
    assert (orr["status"] == 0).all()
    streams = clone(b.streams)
    for s in streams:                                           # the library is not told any size
        s.dst_off, s.dst_cap, s.decom_len = 0, NO_BOUND, 0
    want_total = 0
    for ln in orr["dst_len"]:
        want_total = (want_total + 15) // 16 * 16 + int(ln)
    c = ctx()
    d_src = c.malloc(b.src.nbytes)
    c.h2d(d_src, b.src)
    res = c.measure_batch_device(streams, d_src, b.src.nbytes)
    total = layout_from_results(streams, res, align=16)
    assert total == want_total
    d_dst = c.malloc(total)
    plan = Plan(c, streams)
    try:
        plan.execute(d_src, d_dst)
        gr = synth.result_records(plan.results())
        assert (gr["status"] == 0).all() and np.array_equal(gr["dst_len"], orr["dst_len"])
        out = c.d2h(d_dst, total)
        for i in range(n):
            a, o, ln = int(streams[i].dst_off), int(osr["dst_off"][i]), int(orr["dst_len"][i])
            assert a % 16 == 0 and streams[i].dst_cap == ln
            assert np.array_equal(out[a:a + ln], o_dst[o:o + ln]), i
    finally:
        plan.close()
        c.free(d_dst)
        c.free(d_src)


# ------------------------------------------------------------------------------------------------ 5. linked LZ4 blocks in one batch


def test_linked_lz4_blocks_measured_as_one_batch():
    """Blocks of a linked frame can only be decoded in order, but their sizes do not depend on the history's bytes: one batch, aux0 = the running
    history.  The generator states the whole output; a block's own length is what the oracle decodes the block to on its own (bytes in front of a
    stream read as zeros, E2 -- they change bytes, never lengths)."""
    blocks, expect = FC.lz4_linked_blocks(11, 40, 30000)
    own = [O.decode_stream(A.FMT_LZ4_BLOCK, blk, cap=1 << 20)[1] for blk in blocks]
    assert all(r.status == A.ST_OK for r in own) and sum(r.dst_len for r in own) == len(expect)
    items, hist = [], 0
    for blk, r in zip(blocks, own):
        items.append(dict(fmt=A.FMT_LZ4_BLOCK, src=blk, cap=1 << 20, aux0=hist))
        hist += r.dst_len
    streams, src, _ = pack_streams(items)
    for exact in (1, 0):
        ctx().set_exact_kernels(exact)
        try:
            gr = synth.result_records(ctx().measure_batch(streams, src))
        finally:
            ctx().set_exact_kernels(0)
        assert (gr["status"] == 0).all()
        assert [int(x) for x in gr["dst_len"]] == [r.dst_len for r in own] and [int(x) for x in gr["src_used"]] == [len(blk) for blk in blocks]


# ------------------------------------------------------------------------------------------------ 6. containers


def lib_measure(container, data, limit):
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    o = A.ContainerOptions()
    o.big_endian = 1
    rc = load().alz_container_measure(F._context().h, container, C.byref(o), data, len(data), limit, C.byref(dl), C.byref(su), C.byref(st))
    return rc, st.value, dl.value, su.value


def oracle_outcome(container, data, cap, with_bytes=False):
    data = bytes(data)
    dst = C.create_string_buffer(max(cap, 1))
    dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
    rc = O.lib.oracle_container_decompress(container, C.byref(O._opt(True, None)), data, len(data), dst, cap, C.byref(dl), C.byref(su), C.byref(st))
    return (rc, st.value, dl.value, su.value) + ((dst.raw[:dl.value],) if with_bytes else ())


def content_checksums_made_right(case, data, cap):
    """`data` with every LZ4 CONTENT checksum the in-order reader fails on rewritten to the hash of what the frame decodes to: the file whose outcome
    alz_container_measure reports by definition (it takes content checksums as correct: they need the bytes).  The oracle stops AT a checksum it
    refuses (src_used), with the frame's bytes produced: the frame's start is one of the block starts the generator recorded.  A block checksum
    covers stored bytes, so no hash of output repairs it: such a file is returned as it is, and measure has to refuse it too."""
    data = bytearray(data)
    for _ in range(4):
        rc, _, dl, su, out = oracle_outcome(CT[case.container], data, cap, with_bytes=True)
        if rc != A.E_CHECKSUM or su + 4 > len(data):
            break
        for k in [0] + sorted(set(case.mids)):
            if k > dl:
                continue
            trial = bytearray(data)
            trial[su:su + 4] = O.xxh32(out[k:dl]).to_bytes(4, "little")
            r2 = oracle_outcome(CT[case.container], trial, cap)
            if r2[0] != A.E_CHECKSUM or r2[3] > su:
                data = trial
                break
        else:
            break
    return bytes(data)


def container_difference(container, data, limit, expected=None, where=""):
    """alz_container_measure against the outcome of the oracle's Decompress into `limit` bytes: rc; then status and size; then src_used wherever it is
    defined (every status but OUTPUT_CAPACITY).  Returns a description of the first difference, or None."""
    g = lib_measure(container, data, limit)
    o = expected if expected is not None else oracle_outcome(container, data, limit)
    where = "%s limit=%d" % (where, limit)
    if g[0] != o[0]:
        return "%s: rc %d, oracle %d (status %d / %d, size %d / %d)" % (where, g[0], o[0], g[1], o[1], g[2], o[2])
    if g[0] not in (0, A.E_STREAM):
        return None
    if (g[1], g[2]) != (o[1], o[2]):
        return "%s: status/size %d/%d, oracle %d/%d" % (where, g[1], g[2], o[1], o[2])
    if o[1] != A.ST_OUTPUT_CAPACITY and g[3] != o[3]:
        return "%s: src_used %d, oracle %d (status %d)" % (where, g[3], o[3], o[1])
    return None


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.label for c in CASES])
def test_container_measure_generated_case(i):
    case = CASES[i]
    n = len(case.expect)
    rc, st, size, su = lib_measure(CT[case.container], case.data, NO_BOUND)
    assert (rc, st, size) == (0, A.ST_OK, n), "%r: rc %d status %d size %d of %d" % (case, rc, st, size, n)
    rng = FC.random.Random(case.seed)
    j = rng.randrange(len(case.mids)) if case.mids else 0
    mid = (case.mids[j] + 1) if case.mids else 0
    bad = [e for lim in sorted({n + 4096, n, max(n - 1, 0), 0, min(mid, n)}) for e in [container_difference(CT[case.container], case.data, lim, where=repr(case))] if e]
    assert not bad, bad[:5]
    if n:
        assert lib_measure(CT[case.container], case.data, n - 1)[:2] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY)


def test_container_measure_many_tiny_blocks():
    case = FC.many_tiny_blocks(O.xxh32)
    assert lib_measure(A.C_LZ4_FRAME, case.data, NO_BOUND)[:3] == (0, A.ST_OK, len(case.expect))
    for lim in (len(case.expect), len(case.expect) - 1, 7):
        assert container_difference(A.C_LZ4_FRAME, case.data, lim, where="many tiny blocks") is None


@pytest.mark.parametrize("container", [A.C_PRS, A.C_LZO, A.C_FASTLZ])
def test_container_measure_single_body_files(container, test_bmp):
    for off, size, q in [(0, 10, 4), (0, 10240, 8), (4096, 65536, 0), (100000, 262144, 8), (500000, 70000, 12)]:
        data = O.container_compress(container, test_bmp[off:off + size], quality=q)
        assert lib_measure(container, data, NO_BOUND)[:3] == (0, A.ST_OK, size)
        for lim in (size + 100, size, size - 1, size // 2, 0):
            assert container_difference(container, data, lim, where="container %d size %d" % (container, size)) is None
        if container != A.C_PRS:       # (PRS.Decompress reads a failed file again in the other byte order, PRS.cs:42-57: the oracle decides, above)
            assert lib_measure(container, data, size - 1)[:2] == (A.E_STREAM, A.ST_OUTPUT_CAPACITY)
        for cut in (len(data) // 2, len(data) - 1):
            assert container_difference(container, data[:cut], size + 100, where="container %d truncated" % container) is None
    assert lib_measure(A.C_LZ10, b"\x10\x04\x00\x00\x00abcd", 100)[0] == A.E_UNSUPPORTED


def _stored_bit_toggled(what):
    """a mutant label of the form 'size@OFFSET 0xOLD->0xNEW' whose two values differ in the stored bit alone"""
    m = re.fullmatch(r"size@\d+ (0x[0-9a-f]+)->(0x[0-9a-f]+)", what)
    return bool(m) and int(m.group(1), 16) ^ int(m.group(2), 16) == 0x80000000


def test_container_measure_mutants():
    """All mutants of the generated cases.  Where measure and decompress may differ is decided by how a mutant was MADE: a flipped content checksum
    (measure takes it as correct: expected = the unmutated file's outcome), and a flipped body byte in the three files whose frames carry a content
    checksum and no block checksums (a flip inside a literal changes bytes and not the size): compared unless the oracle ends in E_CHECKSUM.

    Two more kinds of mutant reach the same two situations by another road, in the six files whose frames carry a content checksum: a DOUBLED
    EndMark (the second zero word is read as the content checksum: a wrong checksum over unchanged bytes) and a block size with its STORED bit
    toggled (the block's bytes change, block checksums -- over the stored bytes -- still hold).  The in-order reader ends them in E_CHECKSUM at the
    content checksum; a size query that takes that checksum as correct cannot.  They are not left out: their expected outcome is the oracle's on the
    same file with that checksum field made right (content_checksums_made_right), at every limit.  Rehearsed on the CPU with the oracle standing in
    for the measure kernels: 5 such mutants at the default seed, every other of the 492 compares directly."""
    bad, left_out, repaired, total = [], 0, 0, 0
    with_content_checksum = {c.label for c in CASES if any(fl[0] == "csum" for fl in c.fields)}
    assert len(with_content_checksum) == 6 and set(CHECKSUM_ONLY_CASES) <= with_content_checksum
    for i, case in enumerate(CASES):
        rng = FC.random.Random(FC.SEED * 7919 + i)
        for mu in FC.mutants(case, FC.SEED * 7919 + i):
            total += 1
            what = mu.label[len(case.label) + 3:]
            ample = len(case.expect) + (1 << 20)
            base = case.data if what.startswith("flip csum") else mu.data
            if case.label in with_content_checksum and (what.startswith("EndMark doubled") or _stored_bit_toggled(what)):
                fixed = content_checksums_made_right(case, mu.data, ample)
                repaired += fixed != mu.data
                base = fixed
            o = oracle_outcome(CT[mu.container], base, ample)
            if what.startswith("flip body byte") and case.label in CHECKSUM_ONLY_CASES and o[0] == A.E_CHECKSUM:
                left_out += 1
                continue
            n = o[2]
            for lim in sorted({ample, n, max(n - 1, 0), 0, rng.randrange(n + 1)}):
                e = container_difference(CT[mu.container], mu.data, lim, expected=oracle_outcome(CT[mu.container], base, lim), where=repr(mu))
                if e:
                    bad.append(e)
    print("container mutants: %d, left out (body flips that end in a content checksum error): %d, compared against the file with its content checksum made right: %d"
          % (total, left_out, repaired))
    assert left_out <= 9 and repaired <= 12
    assert not bad, (len(bad), bad[:8])


# ------------------------------------------------------------------------------------------------ 7. Python classes


def _six_files(test_bmp):
    raw = test_bmp[:200000]
    pick = lambda ct: next(c for c in CASES if c.container == ct and len(c.expect) < (4 << 20))      # noqa: E731
    return [(F.PRS(), O.container_compress(A.C_PRS, raw)), (F.LZO(), O.container_compress(A.C_LZO, raw)), (F.FastLZ(), O.container_compress(A.C_FASTLZ, raw)),
            (F.LZ4(), pick("lz4").data), (F.LZ4Legacy(), pick("legacy").data), (F.Snappy(), pick("snappy").data)]


def test_measure_decompressed_size_of_the_six_classes(test_bmp):
    for cls, data in _six_files(test_bmp):
        out = cls.Decompress(data)
        assert cls.MeasureDecompressedSize(data) == len(out), type(cls).__name__
        assert cls.MeasureDecompressedSize(data, limit=len(out)) == len(out)
        with pytest.raises(BufferError):
            cls.MeasureDecompressedSize(data, limit=len(out) - 1)
    with pytest.raises(F.EndOfStreamException):
        F.LZO().MeasureDecompressedSize(O.container_compress(A.C_LZO, test_bmp[:50000])[:-20])
    with pytest.raises(NotImplementedError):
        F.LZ10().MeasureDecompressedSize(b"\x10\x04\x00\x00\x00abcd")


@pytest.mark.parametrize("name", ["PRS", "LZO"])
def test_decompress_measures_instead_of_growing(name, monkeypatch):
    """A stream that expands more than 8 : 1 (one long run): Decompress tries its first guess, measures once, and decodes into exactly that size."""
    cls = getattr(F, name)()
    raw = b"\x5A" * 3000000
    data = O.container_compress(cls.container, raw)
    assert len(data) * 8 < len(raw) and max(len(data) * 8, 1 << 16) < len(raw)
    caps = []
    orig = F._Format.Decompress

    def spy(self, d, capacity=None):
        if capacity is not None:
            caps.append(capacity)
        return orig(self, d, capacity)
    monkeypatch.setattr(F._Format, "Decompress", spy)
    assert cls.Decompress(data) == raw
    assert len(caps) == 2 and caps[1] == len(raw) == cls.MeasureDecompressedSize(data), caps
