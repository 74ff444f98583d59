"""-m gpu: what the batch entry points of the measure, RLE30 / HUF20, aPLib and CRILAYLA / ALLZ families have in common -- the empty batch, the
refusals in front of any upload, the grouping per kind, host form against device form, which bytes a host form downloads -- through the C ABI
itself, once per entry point.  What a stream decodes to is the business of test_gpu_measure / _rlh / _aplib / _bitlz; here every stream of a
batch is compared with the same stream run alone and, where the golden files state one, with its known answer.  Every comparison is exact."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

import rlh_ref as R
from auroralib.compression_amd import _abi as A
from auroralib.compression_amd._lib import AlzError, check
from cases import prose_like
from gpu_common import ctx

pytestmark = pytest.mark.gpu
GUARD = 0xA5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# kinds: the values `format` may take (None: the family ignores it); dst: the family writes a destination; props: alz_lz_properties in front of n
Family = collections.namedtuple("Family", "kinds dst props")
FAMILIES = {"measure": Family(A.FMT_COUNT, False, True), "rlh_decode": Family(A.RLH_COUNT, True, False), "rlh_encode": Family(A.RLH_COUNT, True, False),
            "aplib_decode": Family(None, True, False), "aplib_measure": Family(None, False, False), "bitlz_decode": Family(A.BITLZ_COUNT, True, False)}
EntryPoint = collections.namedtuple("EntryPoint", "name family device")
ENTRY_POINTS = [EntryPoint("alz_%s_batch%s" % (fam, "_device" if device else ""), fam, device) for fam in FAMILIES for device in (False, True)]
HOST_FORMS = [ep for ep in ENTRY_POINTS if not ep.device]
by_name = pytest.mark.parametrize("ep", ENTRY_POINTS, ids=[ep.name for ep in ENTRY_POINTS])
MODES = ((1, 0, "exact"), (0, 1, "variant"), (0, 0, "default"))                  # (alz_ctx_set_exact_kernels, alz_ctx_set_kernel_variant)


# ---------------------------------------------------------------------------------------------- streams
def kat(file, name):
    with open(os.path.join(GOLD, file)) as f:
        return next(c for c in json.load(f)["cases"] if c["name"].startswith(name))


def item(fmt, src, cap, decom_len=0, aux0=0, want=None):
    """want: (status, dst_len, output bytes or None) where a golden file or a restatement states it"""
    return dict(fmt=fmt, src=bytes(src), cap=cap, decom_len=decom_len, aux0=aux0, want=want)


def kat_item(file, name, fmt):
    c = kat(file, name)
    if "expect_len" in c:                                                          # (tests/golden/kat_<format>.json: the streams of alz_format)
        return item(fmt, bytes.fromhex(c["src"]), c["expect_len"], c["decom_len"], c["aux0"], (A.ST_OK, c["expect_len"], None))
    aux0 = A.allz_aux0(*c["params"]) if c.get("params") else c.get("aux0", 0)
    return item(fmt, bytes.fromhex(c["src"]), c["cap"], c.get("decom_len") or 0, aux0, (c["status"], c["dst_len"], bytes.fromhex(c["out"])[:c["dst_len"]]))


def cut(it, num, den):
    """the front num / den of a stream: another length, another answer (the one the stream gives alone)"""
    return dict(it, src=it["src"][:len(it["src"]) * num // den], want=None)


def five(first, last):
    """kinds {first, last, first, last, last}; inside a kind the later stream is the longer one, so the grouped order is not the caller's"""
    batch = [cut(first, 1, 2), cut(last, 2, 3), first, cut(last, 1, 3), last]
    assert len({len(it["src"]) for it in batch if it["fmt"] == first["fmt"]}) >= 2 and len({len(it["src"]) for it in batch[1::2] + batch[4:]}) == 3
    return batch


def raw_item(n, seed, room=8):
    d = prose_like(n, seed) + bytes(n // 3)
    enc = R.rle30_encode(d)
    return item(A.RLH_RLE30, d, len(enc) + room, 0, 0, (A.ST_OK, len(enc), enc) if room >= 0 else (A.ST_OUTPUT_CAPACITY, 0, b""))


_BATCHES = {}


def batch_of(family):
    """the family's batch of five, built once"""
    if not _BATCHES:
        apl = kat_item("aplib_kat.json", "every token kind", 77)
        _BATCHES.update({
            "measure": five(kat_item("kat_lzss.json", "default geometry", A.FMT_LZSS), kat_item("kat_hig.json", "forms A", A.FMT_HIG)),
            "rlh_decode": five(kat_item("rlh_kat.json", "rle30 literal run of 128", A.RLH_RLE30), kat_item("rlh_kat.json", "huf20 a code longer than a word", A.RLH_HUF20_8)),
            "rlh_encode": [raw_item(n, n) for n in (40, 300, 17, 200, 120)],                 # (HUF20 has no encoder: one kind, five lengths)
            "aplib_decode": five(apl, dict(apl, fmt=0xFFFFFFFF)),                            # (`format` is ignored: one group)
            "bitlz_decode": five(kat_item("bitlz_kat.json", "crilayla: literals, a match", A.BITLZ_CRILAYLA), kat_item("bitlz_kat.json", "allz: runs, matches", A.BITLZ_ALLZ))})
        _BATCHES["aplib_measure"] = _BATCHES["aplib_decode"]
        assert A.FMT_LZSS == 0 and A.FMT_HIG == A.FMT_COUNT - 1 and A.RLH_HUF20_8 == A.RLH_COUNT - 1 and A.BITLZ_ALLZ == A.BITLZ_COUNT - 1
    return _BATCHES[family]


def pack(items, dst=True):
    """(streams, src array, dst_bytes): sources 16 bytes apart at least, 16 guard bytes around every destination span.  dst False: the family has
    no destination and must not look at dst_off"""
    streams = (A.Stream * len(items))()
    chunks, so, do = [], 0, 16
    for i, it in enumerate(items):
        streams[i] = A.Stream(so, do if dst else 0xFFFF0000 + i, len(it["src"]), it["cap"], it["decom_len"], it["aux0"], 0, it["fmt"])
        chunks.append(it["src"] + bytes(16 - len(it["src"]) % 16))
        so += len(chunks[-1])
        do = (do + it["cap"] + 16 + 15) // 16 * 16
    return streams, np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy(), do + 64


def clone(streams):
    out = (A.Stream * len(streams))()
    C.memmove(out, streams, C.sizeof(out))
    return out


# ---------------------------------------------------------------------------------------------- calls
def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def invoke(ep, n, streams, src, src_bytes, dst, dst_bytes):
    fam = FAMILIES[ep.family]
    res = (A.Result * n)()
    args = [ctx().h] + ([None] if fam.props else []) + [n, src, src_bytes, streams] + ([dst, dst_bytes] if fam.dst else []) + [res]
    check(getattr(ctx().lib, ep.name)(*args))
    return res


def run(ep, streams, src, dst_bytes, n=None, error=None):
    """One call on a destination full of guard bytes -> (results, the destination afterwards or None, alz_last_kernel_ms).  The host form gets host
    arrays, the device form device buffers.  error: the call must be refused with this code (results None)."""
    n = len(streams) if n is None else n
    c, has_dst = ctx(), FAMILIES[ep.family].dst

    def call(s, d):
        if error is None:
            return invoke(ep, n, streams, s, src.nbytes, d, dst_bytes)
        with pytest.raises(AlzError) as e:
            invoke(ep, n, streams, s, src.nbytes, d, dst_bytes)
        assert e.value.code == error, (ep.name, e.value.code)
        return None
    if not ep.device:
        dst = np.full(dst_bytes, GUARD, dtype=np.uint8)
        res = call(vp(src), vp(dst))
        return res, dst if has_dst else None, c.last_kernel_ms()
    d_src, d_dst = c.malloc(src.nbytes), c.malloc(dst_bytes) if has_dst else None
    try:
        c.h2d(d_src, src)
        if has_dst:
            c.memset(d_dst, GUARD, dst_bytes)
        res = call(d_src, d_dst)
        ms = c.last_kernel_ms()
        return res, c.d2h(d_dst, dst_bytes) if has_dst else None, ms
    finally:
        c.free(d_src)
        if has_dst:
            c.free(d_dst)


def span(s, r):
    """[a, b) of the destination that holds a stream's dst_len bytes: a CRILAYLA stream's end at dst_off + dst_cap"""
    a = s.dst_off + (s.dst_cap - r.dst_len if s.format == A.BITLZ_CRILAYLA else 0)
    return a, a + r.dst_len


def outcome(ep, streams, res, dst):
    """per stream (status, dst_len, src_used, written bytes or None)"""
    out = []
    for i, r in enumerate(res):
        a, b = span(streams[i], r) if ep.family == "bitlz_decode" else (streams[i].dst_off, streams[i].dst_off + r.dst_len)
        out.append((r.status, r.dst_len, r.src_used, dst[a:b].tobytes() if dst is not None else None))
    return out


_FIVE = {}


def five_run(ep):
    """the family's batch of five through `ep`, once: (streams, results, destination, outcome per stream, ms)"""
    if ep.name not in _FIVE:
        streams, src, dst_bytes = pack(batch_of(ep.family), FAMILIES[ep.family].dst)
        res, dst, ms = run(ep, streams, src, dst_bytes)
        _FIVE[ep.name] = (streams, res, dst, outcome(ep, streams, res, dst), ms)
    return _FIVE[ep.name]


# ---------------------------------------------------------------------------------------------- the empty batch
@by_name
def test_empty_batch(ep):
    streams, src, dst_bytes = pack(batch_of(ep.family), FAMILIES[ep.family].dst)
    assert run(ep, streams, src, dst_bytes)[2] > 0                                   # (the call in front leaves a device time behind)
    res, dst, ms = run(ep, (A.Stream * 0)(), src, dst_bytes, n=0)
    assert len(res) == 0 and (dst is None or (dst == GUARD).all())
    # the device forms, alz_measure_batch and alz_bitlz_decode_batch always reset the time in front of their n == 0 return; for the host forms of
    # the RLE30 / HUF20 and aPLib families this line is new with the shared core (they returned first and left the previous call's value)
    assert ms == 0


# ---------------------------------------------------------------------------------------------- refusals in front of any upload or launch
@by_name
def test_source_range_beyond_src_bytes(ep):
    streams, src, dst_bytes = pack(batch_of(ep.family), FAMILIES[ep.family].dst)
    streams[3].src_off = src.nbytes - streams[3].src_len + 1
    _, dst, _ = run(ep, streams, src, dst_bytes, error=A.E_INVALID)
    assert dst is None or (dst == GUARD).all()


@pytest.mark.parametrize("ep", [ep for ep in ENTRY_POINTS if FAMILIES[ep.family].dst], ids=lambda ep: ep.name)
def test_destination_range_beyond_dst_bytes(ep):
    streams, src, dst_bytes = pack(batch_of(ep.family))
    streams[3].dst_off = dst_bytes - streams[3].dst_cap + 1
    _, dst, _ = run(ep, streams, src, dst_bytes, error=A.E_INVALID)
    assert (dst == GUARD).all()


@by_name
def test_unknown_kind(ep):
    fam = FAMILIES[ep.family]
    streams, src, dst_bytes = pack(batch_of(ep.family), fam.dst)
    if fam.kinds is not None:
        streams[1].format = fam.kinds                                                # alz_*_COUNT: one behind the last kind
        _, dst, _ = run(ep, streams, src, dst_bytes, error=A.E_INVALID)
        assert dst is None or (dst == GUARD).all()
        return
    zero = clone(streams)                                                            # aPLib: any value, and the answer of format 0
    for s in zero:
        s.format = 0
    assert {s.format for s in streams} == {77, 0xFFFFFFFF}
    res, dst, _ = run(ep, zero, src, dst_bytes)
    assert outcome(ep, zero, res, dst) == five_run(ep)[3]


# ---------------------------------------------------------------------------------------------- grouping: result i belongs to stream i
@by_name
def test_absent_kinds_and_grouped_order(ep):
    items, fam = batch_of(ep.family), FAMILIES[ep.family]
    streams, res, dst, got, ms = five_run(ep)
    assert ms > 0
    if fam.kinds is not None and ep.family != "rlh_encode":
        assert [s.format for s in streams] == [0, fam.kinds - 1, 0, fam.kinds - 1, fam.kinds - 1]
    written = np.zeros(dst.size if dst is not None else 0, dtype=bool)
    for i, it in enumerate(items):
        s1, src1, dst_bytes1 = pack([it], fam.dst)
        r1, d1, _ = run(ep, s1, src1, dst_bytes1)
        alone = outcome(ep, s1, r1, d1)[0]
        assert got[i] == alone, "%s: stream %d of the batch %r, alone %r" % (ep.name, i, got[i][:3], alone[:3])
        if it["want"] is not None:
            status, dst_len, out = it["want"]
            assert got[i][:2] == (status, dst_len), (ep.name, i, got[i][:3])
            if out is not None and fam.dst:
                assert got[i][3] == out, (ep.name, i)
        if dst is not None:
            a = span(streams[i], res[i])[0] if ep.family == "bitlz_decode" else streams[i].dst_off
            written[a:a + res[i].dst_len] = True
    assert len({g[:3] for g in got}) >= 3                                            # (answers that differ: a result in the wrong place shows)
    if dst is not None and not ep.device:                                            # a host form downloads the streams' bytes and nothing else
        assert (dst[~written] == GUARD).all()


@pytest.mark.parametrize("host", HOST_FORMS, ids=lambda ep: ep.name)
def test_host_form_against_device_form(host):
    device = next(ep for ep in ENTRY_POINTS if ep.device and ep.family == host.family)
    assert five_run(host)[3] == five_run(device)[3]


# ---------------------------------------------------------------------------------------------- which bytes a host form downloads
def test_rlh_encode_downloads_only_streams_that_are_ok():
    items = [raw_item(200, 5, room=-1), raw_item(150, 6)]
    streams, src, dst_bytes = pack(items)
    ep = next(ep for ep in HOST_FORMS if ep.family == "rlh_encode")
    res, dst, _ = run(ep, streams, src, dst_bytes)
    assert (res[0].status, res[0].dst_len) == (A.ST_OUTPUT_CAPACITY, 0)
    assert (res[1].status, res[1].dst_len, res[1].src_used) == (A.ST_OK, len(items[1]["want"][2]), len(items[1]["src"]))
    a = streams[1].dst_off
    assert dst[a:a + res[1].dst_len].tobytes() == items[1]["want"][2]
    dst[a:a + res[1].dst_len] = GUARD
    assert (dst == GUARD).all()                                                      # the failed stream's span included


def test_rlh_decode_downloads_what_a_failed_stream_produced():
    it = kat_item("rlh_kat.json", "rle30 token beyond dst_cap", A.RLH_RLE30)
    assert it["want"][:2] == (A.ST_OUTPUT_CAPACITY, 4)
    streams, src, dst_bytes = pack([it])
    ep = next(ep for ep in HOST_FORMS if ep.family == "rlh_decode")
    res, dst, _ = run(ep, streams, src, dst_bytes)
    assert (res[0].status, res[0].dst_len) == (A.ST_OUTPUT_CAPACITY, 4)
    a = streams[0].dst_off
    assert dst[a:a + 4].tobytes() == it["want"][2] and (dst[:a] == GUARD).all() and (dst[a + 4:] == GUARD).all()


def test_crilayla_bytes_end_at_the_top_of_the_span():
    it = kat_item("bitlz_kat.json", "crilayla: literals, a match", A.BITLZ_CRILAYLA)
    assert it["cap"] == 64 and it["want"][:2] == (A.ST_OK, 23)
    streams, src, dst_bytes = pack([it])
    ep = next(ep for ep in HOST_FORMS if ep.family == "bitlz_decode")
    res, dst, _ = run(ep, streams, src, dst_bytes)
    assert (res[0].status, res[0].dst_len, res[0].src_used) == (A.ST_OK, 23, len(it["src"]))
    top = streams[0].dst_off + 64
    assert dst[top - 23:top].tobytes() == it["want"][2] and (dst[:top - 23] == GUARD).all() and (dst[top:] == GUARD).all()


# ---------------------------------------------------------------------------------------------- the context's mode reaches the launch
@pytest.mark.parametrize("ep", [ep for ep in ENTRY_POINTS if ep.family == "aplib_decode"], ids=lambda ep: ep.name)
def test_aplib_kernel_selection(ep):
    it = kat_item("aplib_kat.json", "every token kind", 0)
    streams, src, dst_bytes = pack([it])
    for exact, variant, mode in MODES:
        ctx().set_exact_kernels(exact)
        ctx().set_kernel_variant(variant)
        try:
            res, dst, _ = run(ep, streams, src, dst_bytes)
        finally:
            ctx().set_exact_kernels(0)
            ctx().set_kernel_variant(0)
        assert outcome(ep, streams, res, dst)[0] == (A.ST_OK, 26, 13, it["want"][2]), mode
