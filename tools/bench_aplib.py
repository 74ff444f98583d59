"""usage: python tools/bench_aplib.py [--streams 10000] [--size 262144] [--reps 12] [--warmup 3] [--lib PATH] [--skip-far] [--json OUT]
Device time of aPLib decode (alz_aplib_decode_batch_device) per kernel family, on an MI355X:

  batch   `--streams` streams that decode to `--size` bytes each, built from 32 distinct token-level generated streams, repeated: a mix of
          literals, one-byte tokens, short matches, repeats and matches with log-uniform distances up to 64 KiB (all inside the byte phase's
          17-bit distance field)
  far     the same output volume as streams of 1 MiB whose matches reach log-uniformly between 0x20000 and 0x200000 back wherever that
          much output exists (the first 128 KiB of a stream cannot): the tokens that go around the queue
  single  one stream of 1 000 KiB through the host form (alz_aplib_decode_batch: upload, decode, download), wall clock and device time --
          the shape of the reference's Benchmarks.md row (Decompress of 1 000 KiB: 3 122 / 1 315 us on one Ryzen thread)

Protocol: `--warmup` untimed calls, then the median of `--reps` (>= 10) device times (HIP events around the launch, alz_last_kernel_ms); every
stream's status and dst_len are checked against the generator's own count, and the production family's output against the exact family's.
--lib: a libauroralz.so built with other ALZ_APLIB_* settings (the LDS ring size experiment of docs/EXPERIMENTS.md).  Prints one JSON line."""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import aplib_ref as R  # noqa: E402


def gen_stream(rng, size, far):
    """(stream bytes, decoded size, token counts): random tokens until `size` bytes are out, the last token cut to fit"""
    toks, produced, lwm = [], 1, False
    counts = dict(lit=0, one=0, short=0, rep=0, match=0, far=0)
    while produced < size:
        room = size - produced
        k = rng.random()
        if k < 0.30 or room < 4:
            toks.append(("lit", rng.randrange(256))); produced += 1; lwm = False; counts["lit"] += 1
        elif k < 0.38:
            toks.append(("one", rng.randrange(1, 16))); produced += 1; lwm = False; counts["one"] += 1
        elif k < 0.48:
            L = rng.choice((2, 3))
            toks.append(("short", rng.randrange(1, 128), L)); produced += L; lwm = True; counts["short"] += 1
        elif k < 0.55 and not lwm:
            L = min(2 + int(rng.expovariate(1 / 6.0)), room)
            toks.append(("rep", L)); produced += L; lwm = True; counts["rep"] += 1
        else:
            if far and produced > 0x20000:
                d = int(math.exp(rng.uniform(math.log(0x20000), math.log(min(produced, R.W)))))
            else:
                d = int(math.exp(rng.uniform(0, math.log(min(produced, 0xFFFF))))) if produced > 1 else 1
            d = max(1, min(d, produced))
            L = min(2 + R.length_delta(d) + int(rng.expovariate(1 / 10.0)), room)
            if L - R.length_delta(d) < 2:
                continue
            toks.append(("match", d, L)); produced += L; lwm = True
            counts["far" if d > 0x1FFFF else "match"] += 1
    toks.append(("end",))
    return R.assemble(rng.randrange(256), toks), produced, counts


def build_batch(distinct, n, size, far, seed):
    rng = random.Random(seed)
    uniq = [gen_stream(rng, size, far) for _ in range(distinct)]
    pad = [(-len(u[0])) % 256 for u in uniq]
    offs, so = [], 0
    for u, p in zip(uniq, pad):
        offs.append(so)
        so += len(u[0]) + p
    src = np.frombuffer(b"".join(u[0] + bytes(p) for u, p in zip(uniq, pad)) + bytes(64), dtype=np.uint8).copy()
    counts = {k: sum(u[2][k] for u in uniq) for k in uniq[0][2]}
    return uniq, offs, src, counts


def time_batch(ctx, A, uniq, offs, src, n, size, reps, warmup):
    cap = (size + 255) // 256 * 256
    streams = (A.Stream * n)()
    for i in range(n):
        u = i % len(uniq)
        streams[i] = A.Stream(offs[u], i * cap, len(uniq[u][0]), size, 0, 0, 0, 0)
    dst_bytes = n * cap + 64
    d_src, d_dst = ctx.malloc(src.nbytes), ctx.malloc(dst_bytes)
    out = {}
    try:
        ctx.h2d(d_src, src)
        first = {}
        for exact, fam in ((1, "exact"), (0, "production")):
            ctx.set_exact_kernels(exact)
            ctx.set_kernel_variant(0 if exact else 1)
            ctx.memset(d_dst, 0xA5, dst_bytes)
            ms = []
            for r in range(warmup + reps):
                res = ctx.aplib_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
                if r >= warmup:
                    ms.append(ctx.last_kernel_ms())
            for i in range(n):
                assert (res[i].status, res[i].dst_len, res[i].src_used) == (0, uniq[i % len(uniq)][1], len(uniq[i % len(uniq)][0])), (fam, i, res[i].status, res[i].dst_len)
            # the first copy of every distinct stream against the restatement's prefix (4 KiB) and, whole, between the families
            for u in range(min(len(uniq), n)):
                got = ctx.d2h(d_dst, size, offset=u * cap)
                if fam == "exact":
                    first[u] = got
                    want = R.decode(uniq[u][0], 4096)[0]
                    assert got[:4096].tobytes() == want, (fam, u)
                else:
                    assert np.array_equal(got, first[u]), (fam, u)
            med = statistics.median(ms)
            out[fam] = dict(ms=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), gib_s=round(n * size / 2**30 / (med / 1e3), 2))
    finally:
        ctx.set_exact_kernels(0)
        ctx.set_kernel_variant(0)
        ctx.free(d_src)
        ctx.free(d_dst)
    out["in_bytes_per_stream"] = int(sum(len(u[0]) for u in uniq) / len(uniq))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--size", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--skip-far", action="store_true")
    ap.add_argument("--skip-single", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.reps >= 10 or a.streams < 100, "the protocol wants the median of at least 10"
    from auroralib.compression_amd import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd.batch import Context
    result = dict(streams=a.streams, size=a.size, reps=a.reps, lib=a.lib or "in-tree")
    t0 = time.time()
    uniq, offs, src, counts = build_batch(a.distinct, a.streams, a.size, False, 355)
    result["batch_tokens"] = counts
    result["gen_s"] = round(time.time() - t0, 1)
    with Context(0) as ctx:
        result["batch"] = time_batch(ctx, A, uniq, offs, src, a.streams, a.size, a.reps, a.warmup)
        print("batch", json.dumps(result["batch"]), flush=True)
        if not a.skip_far:
            fsize = 1 << 20
            fn = max(1, a.streams * a.size // fsize)
            funiq, foffs, fsrc, fcounts = build_batch(min(8, a.distinct), fn, fsize, True, 356)
            result["far_tokens"] = fcounts
            result["far"] = dict(time_batch(ctx, A, funiq, foffs, fsrc, fn, fsize, a.reps, a.warmup), streams=fn, size=fsize)
            print("far", json.dumps(result["far"]), flush=True)
        if not a.skip_single:
            comp, n, _ = gen_stream(random.Random(357), 1000 << 10, False)
            st = (A.Stream * 1)(A.Stream(0, 0, len(comp), n, 0, 0, 0, 0))
            buf = np.frombuffer(comp + bytes(64), dtype=np.uint8).copy()
            single = {}
            for exact, fam in ((1, "exact"), (0, "production")):
                ctx.set_exact_kernels(exact)
                ctx.set_kernel_variant(0 if exact else 1)
                wall, dev = [], []
                for r in range(a.warmup + a.reps):
                    t = time.perf_counter()
                    dst, res = ctx.aplib_decode_batch(st, buf, n + 64)
                    w = time.perf_counter() - t
                    if r >= a.warmup:
                        wall.append(w * 1e3); dev.append(ctx.last_kernel_ms())
                assert (res[0].status, res[0].dst_len) == (0, n)
                single[fam] = dict(wall_ms=round(statistics.median(wall), 3), kernel_ms=round(statistics.median(dev), 3),
                                   kernel_gib_s=round(n / 2**30 / (statistics.median(dev) / 1e3), 3), in_bytes=len(comp))
            ctx.set_exact_kernels(0)
            ctx.set_kernel_variant(0)
            result["single_1000KiB"] = single
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
