#!/usr/bin/env python3
"""make_host_refusals.py -- what the entry points of csrc/alz_host.cpp answer to calls they refuse: (return code, alz_last_error()) per call.

Every call of the table is refused before anything is launched (or is the empty batch, which returns 0): a NULL argument, an unknown kind, a
range outside the stated sizes, a geometry or a setting the GPU path does not take, a context list that cannot be used.  The buffers are 64
bytes, the batches one to three streams.  No call is in the table that is only safe BECAUSE it is refused (a stream of 2 GiB declared over a
small buffer, say).

run_table(lib, h) issues the calls on context `h` and returns [[name, rc, text], ...]; text is "" where rc is 0 (alz_last_error() keeps the last
refusal).  tests/test_gpu_host_refusals.py replays the table and requires equality with tests/golden/host_refusals.json.

Regenerate (GPU box, on the commit whose answers are to be pinned): python tests/golden/make_host_refusals.py
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "host_refusals.json")
N = 64                                                       # bytes of every buffer
WRAP = 2 ** 64 - 1


def run_table(lib, h):
    from auroralib.compression_amd import _abi as A
    vp = C.c_void_p
    rows, names = [], set()

    def call(name, fn, *args, **kw):
        assert name not in names, name
        names.add(name)
        rc = fn(*args, **kw)
        rows.append([name, rc, lib.alz_last_error().decode("utf-8", "replace") if rc else ""])
        return rc

    def S(src_off=0, dst_off=0, src_len=16, dst_cap=16, decom_len=0, aux0=0, aux1=0, fmt=0):
        return A.Stream(src_off, dst_off, src_len, dst_cap, decom_len, aux0, aux1, fmt)

    def T(*streams):
        return (A.Stream * len(streams))(*streams)

    src, dst = (C.c_uint8 * N)(), (C.c_uint8 * N)()
    res, aux, out = (A.Result * 3)(), (A.EncodeAux * 3)(), (C.c_uint32 * 3)()
    d_src, d_dst = vp(), vp()
    assert lib.alz_device_malloc(h, N, C.byref(d_src)) == 0 and lib.alz_device_malloc(h, N, C.byref(d_dst)) == 0
    h2 = vp()
    assert lib.alz_create(0, C.byref(h2)) == 0               # a second context of the same device: the multi entry points' lists
    lz17 = C.byref(A.LzProperties(17, 4, 3, 0, 0, 1 << 17, 0))        # LZSS outside the GPU path: 17 window bits
    lz_md = C.byref(A.LzProperties(12, 4, 3, 0, 0xFEE, 2048, 0))      # ... and a max_distance the encoder does not take
    ok2 = lambda fmt=0: T(S(0, 0, fmt=fmt), S(16, 16, fmt=fmt))
    try:
        # ---- the families whose arguments are (ctx, [extra,] n, src, src_bytes, streams, [dst, dst_bytes,] results): (host function, kinds, has a destination)
        fam = {
            "alz_decode_batch": (lambda c, n, s, sb, st, d, db, r, lz=None: lib.alz_decode_batch(c, lz, n, s, sb, st, d, db, r), A.FMT_COUNT, True),
            "alz_measure_batch": (lambda c, n, s, sb, st, d, db, r, lz=None: lib.alz_measure_batch(c, lz, n, s, sb, st, r), A.FMT_COUNT, False),
            "alz_measure_batch_device": (lambda c, n, s, sb, st, d, db, r, lz=None: lib.alz_measure_batch_device(c, lz, n, s, sb, st, r), A.FMT_COUNT, False),
            "alz_encode_batch": (lambda c, n, s, sb, st, d, db, r, lz=None, cs=None: lib.alz_encode_batch(c, lz, cs, n, s, sb, st, d, db, r, aux), A.FMT_COUNT, True),
            "alz_encode_batch_device": (lambda c, n, s, sb, st, d, db, r, lz=None, cs=None: lib.alz_encode_batch_device(c, lz, cs, n, s, sb, st, d, db, r, aux), A.FMT_COUNT, True),
        }
        for name, kinds, has_dst in (("alz_rlh_decode_batch", A.RLH_COUNT, True), ("alz_rlh_encode_batch", A.RLH_COUNT, True), ("alz_aplib_decode_batch", 1, True),
                                     ("alz_aplib_measure_batch", 1, False), ("alz_bitlz_decode_batch", A.BITLZ_COUNT, True), ("alz_inflate_decode_batch", 1, True),
                                     ("alz_inflate_measure_batch", 1, False), ("alz_deflate_encode_batch", 1, True)):
            for form in (name, name + "_device"):
                f = getattr(lib, form)
                if name.startswith("alz_deflate"):
                    fam[form] = (lambda c, n, s, sb, st, d, db, r, f=f, level=6, flags=0: f(c, level, flags, n, s, sb, st, d, db, r), kinds, has_dst)
                elif has_dst:
                    fam[form] = (lambda c, n, s, sb, st, d, db, r, f=f: f(c, n, s, sb, st, d, db, r), kinds, has_dst)
                else:
                    fam[form] = (lambda c, n, s, sb, st, d, db, r, f=f: f(c, n, s, sb, st, r), kinds, has_dst)
        for form, (f, kinds, has_dst) in fam.items():
            device = form.endswith("_device")
            s, d = (d_src, d_dst) if device else (src, dst)
            call(form + ": NULL context", f, None, 2, s, N, ok2(), d, N, res)
            call(form + ": NULL streams", f, h, 2, s, N, None, d, N, res)
            call(form + ": NULL results", f, h, 2, s, N, ok2(), d, N, None)
            call(form + ": empty batch", f, h, 0, s, N, None, d, N, None)
            if kinds > 1:
                call(form + ": kind = count at stream 1", f, h, 2, s, N, T(S(), S(16, 16, fmt=kinds)), d, N, res)
                call(form + ": unknown kind and a source range beyond, one stream", f, h, 1, s, N, T(S(49, 0, fmt=kinds)), d, N, res)
            call(form + ": source range one byte beyond at stream 1", f, h, 2, s, N, T(S(), S(49, 16)), d, N, res)
            call(form + ": source offset 2^64 - 1", f, h, 2, s, N, T(S(), S(WRAP, 16)), d, N, res)
            call(form + ": source range beyond at streams 2 and 1 of 3", f, h, 3, s, N, T(S(), S(49, 16), S(50, 32)), d, N, res)
            if has_dst:
                call(form + ": destination range one byte beyond at stream 1", f, h, 2, s, N, T(S(), S(16, 49)), d, N, res)
                call(form + ": destination offset 2^64 - 1", f, h, 2, s, N, T(S(), S(16, WRAP)), d, N, res)
                call(form + ": source and destination beyond, one stream", f, h, 1, s, N, T(S(49, 49)), d, N, res)
                call(form + ": bad destination, then bad source", f, h, 2, s, N, T(S(0, 49), S(49, 16)), d, N, res)
                call(form + ": bad source, then bad destination", f, h, 2, s, N, T(S(49, 0), S(16, 49)), d, N, res)
                if kinds > 1:
                    call(form + ": bad destination, then unknown kind", f, h, 2, s, N, T(S(0, 49), S(16, 16, fmt=kinds)), d, N, res)
                    call(form + ": unknown kind, then bad destination", f, h, 2, s, N, T(S(fmt=kinds), S(16, 49)), d, N, res)
            if kinds > 1:
                call(form + ": bad source, then unknown kind", f, h, 2, s, N, T(S(49, 0), S(16, 16, fmt=kinds)), d, N, res)
                call(form + ": unknown kind, then bad source", f, h, 2, s, N, T(S(fmt=kinds), S(49, 16)), d, N, res)
            if form.startswith("alz_encode_batch"):
                call(form + ": NULL destination", f, h, 2, s, N, ok2(), None, N, res)
                call(form + ": LZSS with 17 window bits", f, h, 2, s, N, ok2(), d, N, res, lz17)
                call(form + ": LZSS with max_distance != 1 << window_bits", f, h, 2, s, N, ok2(), d, N, res, lz_md)
                call(form + ": LZSS with 17 window bits and a bad source", f, h, 2, s, N, T(S(), S(49, 16)), d, N, res, lz17)
                for what, cs in (("quality 16", A.Settings(16, 0, 0, 0)), ("max_window_bits 25", A.Settings(8, 25, 0, 0))):
                    call(form + ": " + what, f, h, 2, s, N, ok2(), d, N, res, None, C.byref(cs))
                    call(form + ": " + what + " and a bad source", f, h, 2, s, N, T(S(), S(49, 16)), d, N, res, None, C.byref(cs))
                    call(form + ": " + what + " and an unknown format", f, h, 2, s, N, T(S(fmt=A.FMT_COUNT), S(16, 16)), d, N, res, None, C.byref(cs))
                    call(form + ": " + what + " and 17 window bits", f, h, 2, s, N, ok2(), d, N, res, lz17, C.byref(cs))
            if form == "alz_decode_batch":
                call(form + ": LZ4 block with aux0 > dst_off", f, h, 2, s, N, T(S(), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)), d, N, res)
                call(form + ": LZ4 history, then unknown format", f, h, 2, s, N, T(S(0, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK), S(16, 16, fmt=A.FMT_COUNT)), d, N, res)
                call(form + ": unknown format, then LZ4 history", f, h, 2, s, N, T(S(fmt=A.FMT_COUNT), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)), d, N, res)
                call(form + ": LZSS with 17 window bits", f, h, 2, s, N, ok2(), d, N, res, lz17)
            if form.startswith("alz_measure_batch"):
                call(form + ": LZSS with 17 window bits", f, h, 2, s, N, T(S(fmt=A.FMT_LZ10), S(16, 16)), d, N, res, lz17)
                call(form + ": LZSS with 17 window bits and a bad source", f, h, 2, s, N, T(S(), S(49, 16)), d, N, res, lz17)
            if form.startswith("alz_rlh_encode_batch"):
                call(form + ": HUF20 at stream 1", f, h, 2, s, N, T(S(), S(16, 16, fmt=A.RLH_HUF20_8)), d, N, res)
                call(form + ": HUF20, then bad source", f, h, 2, s, N, T(S(fmt=A.RLH_HUF20_4), S(49, 16)), d, N, res)
            if form.startswith("alz_rlh_decode_batch"):
                call(form + ": HUF20 decom_len 0x10000000", f, h, 2, s, N, T(S(), S(16, 16, decom_len=A.HUF20_MAX_DECOM, fmt=A.RLH_HUF20_4)), d, N, res)
                call(form + ": HUF20 decom_len, then bad destination", f, h, 2, s, N, T(S(decom_len=A.HUF20_MAX_DECOM, fmt=A.RLH_HUF20_8), S(16, 49)), d, N, res)
            if form.startswith("alz_deflate"):
                call(form + ": level 10", f, h, 2, s, N, ok2(), d, N, res, level=10)
                call(form + ": level -1", f, h, 2, s, N, ok2(), d, N, res, level=-1)
                call(form + ": unknown flag bit", f, h, 2, s, N, ok2(), d, N, res, flags=2)
                call(form + ": level 10 and a NULL context", f, None, 2, s, N, ok2(), d, N, res, level=10)
                call(form + ": level 10 and a bad source", f, h, 2, s, N, T(S(), S(49, 16)), d, N, res, level=10)
                call(form + ": level 10 and an unknown flag bit", f, h, 2, s, N, ok2(), d, N, res, level=10, flags=2)

        # ---- alz_plan_create: the device form of the decoder (no buffer sizes: nothing to hold a range against)
        def plan_create(c, lz, n, st, want_out=True):
            p = vp()
            rc = lib.alz_plan_create(c, lz, n, st, C.byref(p) if want_out else None)
            if rc == 0 and p:
                lib.alz_plan_destroy(c, p)
            return rc
        pc = "alz_plan_create"
        call(pc + ": NULL context", plan_create, None, None, 2, ok2())
        call(pc + ": NULL streams", plan_create, h, None, 2, None)
        call(pc + ": NULL out", plan_create, h, None, 2, ok2(), False)
        call(pc + ": empty batch", plan_create, h, None, 0, None)
        call(pc + ": format = count at stream 1", plan_create, h, None, 2, T(S(), S(16, 16, fmt=A.FMT_COUNT)))
        call(pc + ": LZ4 block with aux0 > dst_off", plan_create, h, None, 2, T(S(), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)))
        call(pc + ": LZ4 history + dst_cap beyond 4 GiB", plan_create, h, None, 2, T(S(), S(16, 2 ** 32, aux0=0xFFFFFF00, fmt=A.FMT_LZ4_BLOCK)))
        call(pc + ": LZ4 history, then unknown format", plan_create, h, None, 2, T(S(0, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK), S(16, 16, fmt=A.FMT_COUNT)))
        call(pc + ": unknown format, then LZ4 history", plan_create, h, None, 2, T(S(fmt=A.FMT_COUNT), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)))
        call(pc + ": LZSS with 17 window bits", plan_create, h, lz17, 2, ok2())
        call(pc + ": LZSS with 17 window bits and an unknown format", plan_create, h, lz17, 2, T(S(), S(16, 16, fmt=A.FMT_COUNT)))
        call(pc + ": 17 window bits without an LZSS stream", plan_create, h, lz17, 0, None)

        # ---- the range families: (ctx, [kind | seed,] n, src, src_bytes, ranges, out)
        rng = {}
        for form in ("alz_checksum_batch", "alz_checksum_batch_device"):
            rng[form] = lambda c, n, s, sb, t, o, f=getattr(lib, form), kind=A.CK_CRC32: f(c, kind, n, s, sb, t, o)
        for form in ("alz_crc32c_batch", "alz_crc32c_batch_device"):
            rng[form] = lambda c, n, s, sb, t, o, f=getattr(lib, form): f(c, n, s, sb, t, o)
        for form in ("alz_xxh32_batch", "alz_xxh32_batch_device"):
            rng[form] = lambda c, n, s, sb, t, o, f=getattr(lib, form): f(c, 5, n, s, sb, t, o)
        for form, f in rng.items():
            s = d_src if form.endswith("_device") else src
            call(form + ": NULL context", f, None, 2, s, N, ok2(), out)
            call(form + ": NULL ranges", f, h, 2, s, N, None, out)
            call(form + ": NULL out", f, h, 2, s, N, ok2(), None)
            call(form + ": empty batch", f, h, 0, s, N, None, None)
            call(form + ": range one byte beyond at range 1", f, h, 2, s, N, T(S(), S(49, 16)), out)
            call(form + ": range offset 2^64 - 1", f, h, 2, s, N, T(S(), S(WRAP, 16)), out)
            call(form + ": ranges 2 and 1 of 3 beyond", f, h, 3, s, N, T(S(), S(49, 16), S(50, 32)), out)
            if form.startswith("alz_checksum"):
                call(form + ": kind 2", f, h, 2, s, N, ok2(), out, kind=2)
                call(form + ": kind 2 and a NULL context", f, None, 2, s, N, ok2(), out, kind=2)
                call(form + ": kind 2 and a range beyond", f, h, 2, s, N, T(S(), S(49, 16)), out, kind=2)
                call(form + ": Adler-32, range one byte beyond", f, h, 1, s, N, T(S(1, 0, 64)), out, kind=A.CK_ADLER32)

        # ---- several contexts
        part = (C.c_uint32 * 3)()
        L = lambda *cs: (vp * len(cs))(*cs)

        def plan_create_multi(ctxs, n_ctx, lz, n, st, part_of, want_out=True):
            mp = vp()
            rc = lib.alz_plan_create_multi(ctxs, n_ctx, lz, n, st, part_of, C.byref(mp) if want_out else None, part)
            if rc == 0 and mp:
                lib.alz_plan_destroy_multi(mp)
            return rc
        multi = {
            "alz_decode_batch_multi": lambda ctxs, k, n, st, lz=None, cs=None, r=res, d=dst: lib.alz_decode_batch_multi(ctxs, k, lz, n, src, N, st, d, N, r, part),
            "alz_encode_batch_multi": lambda ctxs, k, n, st, lz=None, cs=None, r=res, d=dst: lib.alz_encode_batch_multi(ctxs, k, lz, cs, n, src, N, st, d, N, r, aux, part),
            "alz_plan_create_multi": lambda ctxs, k, n, st, lz=None, cs=None, r=res, d=dst: plan_create_multi(ctxs, k, lz, n, st, None),
        }
        for form, f in multi.items():
            call(form + ": NULL context list", f, None, 1, 2, ok2())
            call(form + ": n_ctx 0", f, L(h), 0, 2, ok2())
            call(form + ": n_ctx 65", f, L(*([h] * 65)), 65, 2, ok2())
            call(form + ": NULL context at index 1", f, L(h, None), 2, 2, ok2())
            call(form + ": the same context twice", f, L(h, h), 2, 2, ok2())
            call(form + ": the same context twice, at 0 and 2", f, L(h, h2, h), 3, 2, ok2())
            call(form + ": NULL context at index 2 behind a context listed twice", f, L(h, h, None), 3, 2, ok2())
            call(form + ": NULL streams", f, L(h), 1, 2, None)
            call(form + ": empty batch", f, L(h, h2), 2, 0, None)
            call(form + ": the same context twice and an unknown format", f, L(h, h), 2, 2, T(S(), S(16, 16, fmt=A.FMT_COUNT)))
            call(form + ": format = count at stream 1", f, L(h, h2), 2, 2, T(S(), S(16, 16, fmt=A.FMT_COUNT)))
            if form != "alz_plan_create_multi":
                call(form + ": NULL results", f, L(h), 1, 2, ok2(), r=None)
                call(form + ": source range one byte beyond at stream 1", f, L(h, h2), 2, 2, T(S(), S(49, 16)))
                call(form + ": source offset 2^64 - 1", f, L(h), 1, 2, T(S(), S(WRAP, 16)))
                call(form + ": destination range one byte beyond at stream 1", f, L(h, h2), 2, 2, T(S(), S(16, 49)))
                call(form + ": bad destination, then unknown format", f, L(h, h2), 2, 2, T(S(0, 49), S(16, 16, fmt=A.FMT_COUNT)))
                call(form + ": unknown format, then bad destination", f, L(h, h2), 2, 2, T(S(fmt=A.FMT_COUNT), S(16, 49)))
                call(form + ": bad source, then bad destination", f, L(h), 1, 2, T(S(49, 0), S(16, 49)))
                call(form + ": bad destination, then bad source", f, L(h), 1, 2, T(S(0, 49), S(49, 16)))
        f = multi["alz_decode_batch_multi"]
        call("alz_decode_batch_multi: LZ4 block with aux0 > dst_off", f, L(h, h2), 2, 2, T(S(), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)))
        call("alz_decode_batch_multi: LZ4 history, then bad source", f, L(h), 1, 2, T(S(0, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK), S(49, 16)))
        f = multi["alz_encode_batch_multi"]
        call("alz_encode_batch_multi: NULL destination", f, L(h), 1, 2, ok2(), d=None)
        call("alz_encode_batch_multi: LZSS with 17 window bits", f, L(h), 1, 2, ok2(), lz17)
        call("alz_encode_batch_multi: LZSS with max_distance != 1 << window_bits, two contexts", f, L(h, h2), 2, 2, ok2(), lz_md)
        for what, cs in (("quality 16", A.Settings(16, 0, 0, 0)), ("max_window_bits 25", A.Settings(8, 25, 0, 0))):
            call("alz_encode_batch_multi: " + what, f, L(h), 1, 2, ok2(), None, C.byref(cs))
            call("alz_encode_batch_multi: " + what + " and a bad source", f, L(h), 1, 2, T(S(), S(49, 16)), None, C.byref(cs))
        f = multi["alz_plan_create_multi"]
        call("alz_plan_create_multi: NULL out", plan_create_multi, L(h), 1, None, 2, ok2(), None, False)
        call("alz_plan_create_multi: part_of[1] = n_ctx", plan_create_multi, L(h), 1, None, 2, ok2(), (C.c_uint32 * 2)(0, 1))
        call("alz_plan_create_multi: part_of[0] = n_ctx, two contexts", plan_create_multi, L(h, h2), 2, None, 2, ok2(), (C.c_uint32 * 2)(2, 0))
        call("alz_plan_create_multi: LZ4 block with aux0 > dst_off", f, L(h), 1, 2, T(S(), S(16, 16, aux0=17, fmt=A.FMT_LZ4_BLOCK)))
        call("alz_plan_create_multi: LZSS with 17 window bits", f, L(h, h2), 2, 2, ok2(), lz17)
        call("alz_partition_batch: NULL streams", lib.alz_partition_batch, 2, None, 1, part, None)
        call("alz_partition_batch: no parts", lib.alz_partition_batch, 2, ok2(), 0, part, None)
    finally:
        lib.alz_synchronize(h)
        lib.alz_device_free(h, d_src)
        lib.alz_device_free(h, d_dst)
        lib.alz_destroy(h2)
    return rows


def main():
    sys.path.insert(0, ROOT)
    from auroralib.compression_amd.batch import Context
    with Context(0) as ctx:
        rows = run_table(ctx.lib, ctx.h)
    with open(OUT, "w") as f:
        json.dump(dict(about="(return code, alz_last_error()) of the refused calls of tests/golden/make_host_refusals.py", cases=rows), f, indent=0)
        f.write("\n")
    print("%d calls, %d refused -> %s" % (len(rows), sum(1 for r in rows if r[1]), OUT))


if __name__ == "__main__":
    main()
