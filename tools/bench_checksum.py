"""usage: python tools/bench_checksum.py [--streams 10000] [--size 262144] [--reps 12] [--warmup 3] [--distinct 64] [--level 6] [--threads 16]
                                       [--ladder 16384,32768,65536,131072,262144,1048576] [--big 1073741824] [--loop-files 200] [--json OUT]
Device time of Adler-32 and CRC-32 (alz_checksum_batch_device) on an MI355X, with what it is to be read against, all in one session:

  batch      `--streams` raw buffers of `--size` bytes, device-resident: the raw buffers of synth.py (`--distinct` Yaz0 streams of the seeded
             generator, decoded), compressed on the host with zlib at `--level` and decoded into HBM by alz_inflate_decode_batch_device -- that
             decode is timed too (the inflate kernel on the same batch's compressed form)
  copy       alz_measure_copy_bandwidth: the roofline of a kernel that reads each byte once
  host       zlib.crc32 / zlib.adler32 over the same buffers on `--threads` host threads, wall clock, median of 3
  ladder     both kinds at every chunk size of `--ladder` (alz_debug_checksum_chunk); the default is put back afterwards
  big        ONE range of `--big` bytes (the first buffers of the batch, as one range)
  zfile      alz_zfile_decode_batch on `--streams` ZLib files against a loop of alz_zlib_decompress over `--loop-files` of them, scaled to
             `--streams`: wall clock of one call each, host buffers in and out

Protocol: `--warmup` untimed calls, then the median of `--reps` (>= 10) device times (HIP events around the launches, alz_last_kernel_ms); every
result is checked against the standard library (the big range through alz_checksum_combine over the buffers' sums).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--size", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--ladder", default="16384,32768,65536,131072,262144,1048576")
    ap.add_argument("--big", type=int, default=1 << 30)
    ap.add_argument("--loop-files", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.reps >= 10 or a.streams < 100, "the protocol wants the median of at least 10"
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd import synth
    from auroralib.compression_amd.batch import Context
    from bench_inflate import raw_buffers
    n, size = a.streams, a.size
    kinds = ((A.CK_ADLER32, zlib.adler32, "adler32"), (A.CK_CRC32, zlib.crc32, "crc32"))
    result = dict(streams=n, size=size, reps=a.reps, level=a.level)

    def emit(key, value):
        result[key] = value
        print(key, json.dumps(value), flush=True)

    with Context(0) as ctx:
        lib = ctx.lib
        default_chunk = lib.alz_debug_checksum_chunk(0)
        raws = raw_buffers(ctx, A, synth, min(a.distinct, n), size)
        k = len(raws)
        with ThreadPoolExecutor(a.threads) as pool:
            comps = list(pool.map(lambda d: zlib.compress(d, a.level), raws))      # ZLib files; bytes [2, -4) are the raw DEFLATE body
        want = {name: [ref(d) for d in raws] for _, ref, name in kinds}
        offs, so = [], 0
        for c in comps:
            offs.append(so)
            so += (len(c) + 255) // 256 * 256
        src = np.frombuffer(b"".join(c + bytes((-len(c)) % 256) for c in comps) + bytes(64), dtype=np.uint8).copy()
        cap = (size + 255) // 256 * 256
        streams = (A.Stream * n)()
        for i in range(n):
            u = i % k
            streams[i] = A.Stream(offs[u] + 2, i * cap, len(comps[u]) - 6, size, 0, 0, 0, 0)
        dst_bytes = n * cap + 64
        d_src, d_dst = ctx.malloc(src.nbytes), ctx.malloc(dst_bytes)
        try:
            ctx.h2d(d_src, src)
            emit("copy_gb_s", round(ctx.copy_bandwidth(), 1))

            def timed(call):
                ms = []
                for r in range(a.warmup + a.reps):
                    out = call()
                    if r >= a.warmup:
                        ms.append(ctx.last_kernel_ms())
                return out, statistics.median(ms), min(ms), max(ms)

            def row(med, lo, hi, nbytes):
                return dict(ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), gb_s=round(nbytes / 1e9 / (med / 1e3), 1))

            # the raw buffers into HBM: the inflate kernel on the batch's compressed form
            res, med, lo, hi = timed(lambda: ctx.inflate_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes))
            assert all((r.status, r.dst_len) == (0, size) for r in res)
            emit("inflate_decode", row(med, lo, hi, n * size))

            def run_kinds(tag, ranges, expect, nbytes):
                for kind, _, name in kinds:
                    got, med, lo, hi = timed(lambda: ctx.checksum_batch_device(kind, ranges, d_dst, dst_bytes))
                    assert [int(g) for g in got] == expect(name), (tag, name)
                    emit("%s_%s" % (tag, name), row(med, lo, hi, nbytes))

            run_kinds("batch", streams_as_ranges(A, n, cap, size), lambda name: [want[name][i % k] for i in range(n)], n * size)
            for chunk in [int(x) for x in a.ladder.split(",") if x]:
                assert lib.alz_debug_checksum_chunk(chunk) == chunk
                run_kinds("chunk_%d" % chunk, streams_as_ranges(A, n, cap, size), lambda name: [want[name][i % k] for i in range(n)], n * size)
            lib.alz_debug_checksum_chunk(default_chunk)
            if cap == size and a.big <= n * size:                                  # the buffers lie back to back: the first `big` bytes are one range
                whole, rest = divmod(a.big, size)

                def big_sum(name):
                    kind, ref = next((kd, rf) for kd, rf, nm in kinds if nm == name)
                    v = ref(b"")
                    for i in range(whole):
                        v = lib.alz_checksum_combine(kind, v, want[name][i % k], size)
                    return [lib.alz_checksum_combine(kind, v, ref(raws[whole % k][:rest]), rest)]
                one = (A.Stream * 1)(A.Stream(0, 0, a.big, 0, 0, 0, 0, 0))
                run_kinds("big", one, big_sum, a.big)
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
        # the CPU baseline: the same n buffers through zlib on `threads` host threads
        for _, ref, name in kinds:
            walls = []
            with ThreadPoolExecutor(a.threads) as pool:
                for _r in range(3):
                    t = time.perf_counter()
                    got = list(pool.map(lambda i: ref(raws[i % k]), range(n)))
                    walls.append(time.perf_counter() - t)
                    assert got[:k] == want[name]
            w = statistics.median(walls)
            emit("host_%s" % name, dict(threads=a.threads, ms=round(w * 1e3, 1), gb_s=round(n * size / 1e9 / w, 2)))
        # end to end: n ZLib files in one batched call against a loop of the single-file call
        files = (A.Stream * n)()
        for i in range(n):
            files[i] = A.Stream(offs[i % k], i * size, len(comps[i % k]), size, 0, 0, 0, A.ZFILE_ZLIB)
        dst = np.empty(n * size + 64, dtype=np.uint8)
        for r in range(2):                                                         # (the first call allocates)
            t = time.perf_counter()
            _, fres = ctx.zfile_decode_batch(files, src, dst.nbytes, dst=dst)
            wall = time.perf_counter() - t
        assert all((f.rc, f.dst_len) == (0, size) for f in fres)
        for i in (0, k - 1, n - 1):
            assert dst[i * size:(i + 1) * size].tobytes() == raws[i % k], i
        emit("zfile_batch", dict(files=n, ms=round(wall * 1e3, 1), gb_s=round(n * size / 1e9 / wall, 2)))
        m = min(a.loop_files, n)
        one = np.empty(size, dtype=np.uint8)
        dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()
        for r in range(2):
            t = time.perf_counter()
            for i in range(m):
                c = comps[i % k]
                rc = lib.alz_zlib_decompress(ctx.h, c, len(c), one.ctypes.data_as(C.c_void_p), size, C.byref(dl), C.byref(su), C.byref(st))
                assert rc == 0 and dl.value == size
            wall = time.perf_counter() - t
        emit("zlib_loop", dict(files=m, ms=round(wall * 1e3, 1), scaled_to=n, scaled_ms=round(wall * 1e3 * n / m, 1), gb_s=round(m * size / 1e9 / wall, 3)))
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def streams_as_ranges(A, n, cap, size):
    t = (A.Stream * n)()
    for i in range(n):
        t[i] = A.Stream(i * cap, 0, size, 0, 0, 0, 0, 0)
    return t


if __name__ == "__main__":
    main()
