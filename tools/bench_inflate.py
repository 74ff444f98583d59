"""usage: python tools/bench_inflate.py [--streams 10000] [--size 262144] [--reps 12] [--warmup 3] [--distinct 64] [--level 6] [--threads 16] [--lib PATH] [--json OUT]
Device time of DEFLATE decode and measure (alz_inflate_decode_batch_device, alz_inflate_measure_batch_device) on an MI355X:

  batch   `--streams` raw DEFLATE streams that decode to `--size` bytes each: the raw buffers of synth.py (`--distinct` Yaz0 streams of the
          seeded generator, decoded), compressed on the host with zlib at `--level`, repeated
  host    the same batch through zlib.decompress on `--threads` host threads of the same machine (zlib releases the interpreter lock): the
          CPU baseline, wall clock, median of 3

Protocol: `--warmup` untimed calls, then the median of `--reps` (>= 10) device times (HIP events around the launch on the launch stream,
alz_last_kernel_ms); every stream's status, dst_len and src_used are checked, and the first copy of every distinct stream byte for byte.
--lib: a libauroralz.so built with another ALZ_INFLATE_LW (the LDS ring size experiment of docs/EXPERIMENTS.md).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def raw_buffers(ctx, A, synth, distinct, size):
    b = synth.make_batch(A.FMT_YAZ0, distinct, size, synth.seed_for(15))
    dst, res = ctx.decode_batch(b.streams, b.src, b.dst_bytes)
    assert all(r.status == 0 and r.dst_len == size for r in res)
    return [dst[int(s.dst_off):int(s.dst_off) + size].tobytes() for s in b.streams]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--size", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.reps >= 10 or a.streams < 100, "the protocol wants the median of at least 10"
    from auroralib.compression_amd import _lib
    if a.lib:
        _lib.SO_PATH = os.path.abspath(a.lib)
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd import synth
    from auroralib.compression_amd.batch import Context
    n, size = a.streams, a.size
    result = dict(streams=n, size=size, reps=a.reps, level=a.level, lib=a.lib or "in-tree")
    with Context(0) as ctx:
        raws = raw_buffers(ctx, A, synth, min(a.distinct, n), size)

        def deflate(d):
            c = zlib.compressobj(a.level, zlib.DEFLATED, -15)
            return c.compress(d) + c.flush()
        with ThreadPoolExecutor(a.threads) as pool:
            comps = list(pool.map(deflate, raws))
        result["in_bytes_per_stream"] = int(sum(map(len, comps)) / len(comps))
        offs, so = [], 0
        for c in comps:
            offs.append(so)
            so += (len(c) + 255) // 256 * 256
        src = np.frombuffer(b"".join(c + bytes((-len(c)) % 256) for c in comps) + bytes(64), dtype=np.uint8).copy()
        cap = (size + 255) // 256 * 256
        streams = (A.Stream * n)()
        for i in range(n):
            u = i % len(comps)
            streams[i] = A.Stream(offs[u], i * cap, len(comps[u]), size, 0, 0, 0, 0)
        dst_bytes = n * cap + 64
        d_src, d_dst = ctx.malloc(src.nbytes), ctx.malloc(dst_bytes)
        try:
            ctx.h2d(d_src, src)
            ctx.memset(d_dst, 0xA5, dst_bytes)
            for what in ("decode", "measure"):
                ms = []
                for r in range(a.warmup + a.reps):
                    if what == "decode":
                        res = ctx.inflate_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
                    else:
                        res = ctx.inflate_measure_batch_device(streams, d_src, src.nbytes)
                    if r >= a.warmup:
                        ms.append(ctx.last_kernel_ms())
                for i in range(n):
                    assert (res[i].status, res[i].dst_len, res[i].src_used) == (0, size, len(comps[i % len(comps)])), (what, i, res[i].status, res[i].dst_len)
                med = statistics.median(ms)
                result[what] = dict(ms=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), gib_s=round(n * size / 2**30 / (med / 1e3), 2))
                print(what, json.dumps(result[what]), flush=True)
            for u in range(len(comps)):
                assert ctx.d2h(d_dst, size, offset=u * cap).tobytes() == raws[u], u
            last = (n - 1) % len(comps)
            assert ctx.d2h(d_dst, size, offset=(n - 1) * cap).tobytes() == raws[last]
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
    # the CPU baseline: the same n streams through zlib.decompress on `threads` host threads
    walls = []
    with ThreadPoolExecutor(a.threads) as pool:
        for _ in range(3):
            t = time.perf_counter()
            total = sum(pool.map(lambda i: len(zlib.decompress(comps[i % len(comps)], -15)), range(n)))
            walls.append(time.perf_counter() - t)
            assert total == n * size
    w = statistics.median(walls)
    result["host_zlib"] = dict(threads=a.threads, ms=round(w * 1e3, 1), gib_s=round(n * size / 2**30 / w, 2))
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
