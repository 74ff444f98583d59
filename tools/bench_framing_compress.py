"""usage: python tools/bench_framing_compress.py [--files 2000] [--size 65536] [--distinct 64] [--reps 5] [--qualities 0,8] [--ranges 10000]
                                               [--range-size 65536] [--big 67108864] [--kernel-reps 12] [--warmup 3] [--json OUT]
Batched LZ4 / Snappy file compression and the CRC-32C kernels on an MI355X, with what they are to be read against, all in one session:

  batch / loop   `--files` raw inputs of `--size` bytes of synthetic text (`--distinct` different ones), written as LZ4 frames of 64 KiB blocks
                 and as framed Snappy files, at every quality of `--qualities`.  alz_framing_compress_batch, one call, against a loop of
                 alz_container_compress over the same inputs: wall clock of calls that end synchronised, host buffers in and out.  After one
                 warm-up of each side the two sides ALTERNATE `--reps` times; the medians and their ratio are reported, and the batch's host
                 time per phase (its last run).  The files of the two sides are compared byte for byte.
  crc32c         alz_crc32c_batch_device on `--ranges` ranges of `--range-size` bytes and on ONE range of `--big` bytes, device-resident:
                 `--warmup` untimed calls, then the median of `--kernel-reps` device times (alz_last_kernel_ms); next to them the host CRC-32C
                 of the single-file writer (alz_container.cpp: SSE4.2 where the CPU has it) on one thread over the same bytes.  Every value
                 is checked against the host function.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PHASES = ("layout", "upload", "encode", "crc32c", "settle", "copy", "download")


def text_like(n, seed):
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randrange(2, 10))) for _ in range(200)]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(words) + (b" " if rng.random() < 0.9 else b".\n")
    return bytes(out[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qualities", default="0,8")
    ap.add_argument("--ranges", type=int, default=10000)
    ap.add_argument("--range-size", type=int, default=65536)
    ap.add_argument("--big", type=int, default=64 << 20)
    ap.add_argument("--kernel-reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd.batch import Context
    result = dict(files=a.files, size=a.size, reps=a.reps)

    def emit(key, value):
        result[key] = value
        print(key, json.dumps(value), flush=True)

    with Context(0) as ctx:
        lib = ctx.lib
        lib.alz_debug_host_crc32c.argtypes = [C.c_void_p, C.c_size_t]
        lib.alz_debug_host_crc32c.restype = C.c_uint32
        lib.alz_debug_framing_compress_phases.argtypes = [C.POINTER(C.c_double), C.c_int]
        lib.alz_container_compress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.alz_container_compress_bound.restype = C.c_size_t
        lib.alz_container_compress_bound.argtypes = [C.c_uint32, C.c_size_t]

        k, n, size = min(a.distinct, a.files), a.files, a.size
        texts = [text_like(size, 100 + i) for i in range(k)]
        src = np.frombuffer(b"".join(texts[i % k] for i in range(n)) + bytes(1), dtype=np.uint8)   # every file has a source of its own: the batch uploads them all
        for name, ct, aux0 in (("lz4", A.C_LZ4_FRAME, 0x10000), ("snappy", A.C_SNAPPY, 0)):
            cap = int(lib.alz_container_compress_bound(ct, size))
            slot = (cap + 255) // 256 * 256
            files = (A.Stream * n)()
            for i in range(n):
                files[i] = A.Stream(i * size, i * slot, size, cap, 0, aux0, 0, ct)
            dst = np.empty(n * slot, dtype=np.uint8)
            one = np.empty(cap, dtype=np.uint8)
            opt = A.ContainerOptions()
            opt.chunk_size = aux0
            dl = C.c_size_t()
            for q in [int(x) for x in a.qualities.split(",")]:
                st = A.Settings(q, 0, 0, 0)
                lens, looped = [0] * n, {}

                def batch():
                    t = time.perf_counter()
                    _, res = ctx.framing_compress_batch(files, src, dst.nbytes, dst=dst, quality=q)
                    w = time.perf_counter() - t
                    assert all(r.rc == 0 and r.src_used == size for r in res)
                    for i, r in enumerate(res):
                        lens[i] = r.dst_len
                    return w

                def loop():
                    t = time.perf_counter()
                    for i in range(n):
                        rc = lib.alz_container_compress(ctx.h, ct, C.byref(opt), C.byref(st), texts[i % k], size, one.ctypes.data_as(C.c_void_p), cap, C.byref(dl))
                        assert rc == 0
                        if i < k:
                            looped[i] = one[:dl.value].tobytes()
                    return time.perf_counter() - t
                batch(), loop()                                                    # warm-up: allocations, code objects
                for i in range(n):                                                 # the two sides write the same files
                    assert dst[i * slot:i * slot + lens[i]].tobytes() == looped[i % k], (name, q, i)
                tb, tl = [], []
                for _ in range(a.reps):                                            # the two sides alternate
                    tb.append(batch())
                    tl.append(loop())
                ph = (C.c_double * len(PHASES))()
                lib.alz_debug_framing_compress_phases(ph, len(PHASES))
                mb, ml = statistics.median(tb), statistics.median(tl)
                emit("%s_q%d" % (name, q), dict(
                    files=n, written_bytes=int(sum(lens)),
                    batch_ms=round(mb * 1e3, 2), batch_ms_min=round(min(tb) * 1e3, 2), batch_ms_max=round(max(tb) * 1e3, 2),
                    loop_ms=round(ml * 1e3, 2), loop_ms_min=round(min(tl) * 1e3, 2), loop_ms_max=round(max(tl) * 1e3, 2),
                    loop_over_batch=round(ml / mb, 2), batch_gb_s=round(n * size / 1e9 / mb, 3), loop_gb_s=round(n * size / 1e9 / ml, 3),
                    last_batch_phase_ms={p: round(ph[j], 2) for j, p in enumerate(PHASES)}, last_batch_ms=round(tb[-1] * 1e3, 2)))

        # CRC-32C: many ranges, one long range; the bytes are 16 MiB of random data repeated through the buffer
        unit = np.frombuffer(random.Random(7).randbytes(16 << 20), dtype=np.uint8)
        total = max(a.ranges * a.range_size, a.big)
        total = (total + unit.nbytes - 1) // unit.nbytes * unit.nbytes
        d = ctx.malloc(total)
        try:
            for o in range(0, total, unit.nbytes):
                ctx.h2d(C.c_void_p(d.value + o), unit)

            def host_rate(off, ln, count):
                """CRC-32C of `count` ranges of ln bytes on one host thread: (value of the first, seconds)"""
                tile = np.concatenate([unit] * ((off % unit.nbytes + ln) // unit.nbytes + 2))[off % unit.nbytes:off % unit.nbytes + ln]
                tile = np.ascontiguousarray(tile)
                t = time.perf_counter()
                for _ in range(count):
                    v = lib.alz_debug_host_crc32c(tile.ctypes.data_as(C.c_void_p), ln)
                return v, time.perf_counter() - t

            def timed(ranges):
                ms = []
                for r in range(a.warmup + a.kernel_reps):
                    got = ctx.crc32c_batch_device(ranges, d, total)
                    if r >= a.warmup:
                        ms.append(ctx.last_kernel_ms())
                return got, statistics.median(ms), min(ms), max(ms)

            many = (A.Stream * a.ranges)()
            for i in range(a.ranges):
                many[i] = A.Stream(i * a.range_size, 0, a.range_size, 0, 0, 0, 0, 0)
            got, med, lo, hi = timed(many)
            per_unit = unit.nbytes // a.range_size if a.range_size <= unit.nbytes and unit.nbytes % a.range_size == 0 else 0
            for i in range(min(a.ranges, max(per_unit, 1), 64)):
                assert int(got[i]) == host_rate(i * a.range_size, a.range_size, 1)[0], i
            if per_unit:
                assert all(int(got[i]) == int(got[i % per_unit]) for i in range(a.ranges))
            nbytes = a.ranges * a.range_size
            sample = min(a.ranges, 1000)
            _, hs = host_rate(0, a.range_size, sample)
            emit("crc32c_many", dict(ranges=a.ranges, range_size=a.range_size, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                     gb_s=round(nbytes / 1e9 / (med / 1e3), 1), host_one_thread_gb_s=round(sample * a.range_size / 1e9 / hs, 2)))
            big = (A.Stream * 1)(A.Stream(5, 0, a.big - 5, 0, 0, 0, 0, 0))
            got, med, lo, hi = timed(big)
            hv, hs = host_rate(5, a.big - 5, 1)
            assert int(got[0]) == hv
            emit("crc32c_one_range", dict(bytes=a.big - 5, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                          gb_s=round((a.big - 5) / 1e9 / (med / 1e3), 1), host_one_thread_gb_s=round((a.big - 5) / 1e9 / hs, 2)))
        finally:
            ctx.free(d)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
