"""usage: python tools/bench_framed.py [--files 2000] [--size 65536] [--distinct 64] [--reps 5] [--ranges 10000] [--range-size 262144] [--big 67108864]
                                     [--kernel-reps 12] [--warmup 3] [--json OUT]
Batched LZ4 / Snappy file decode and the XXH32 kernel on an MI355X, with what they are to be read against, all in one session:

  batch / loop   `--files` LZ4 frames (BD 4, content checksum set) and as many framed Snappy files, each `--size` bytes of synthetic text
                 (`--distinct` different ones), written by the library's own Compress -- the LZ4 frames get FLG bit 2 and the XXH32 of their
                 content afterwards, since Compress never writes one.  alz_framed_decode_batch, one call, against a loop of
                 alz_container_decompress over the same files: wall clock of calls that end synchronised, host buffers in and out.  After one
                 warm-up of each side the two sides ALTERNATE `--reps` times; the medians and their ratio are reported.
  xxh32          alz_xxh32_batch_device on `--ranges` ranges of `--range-size` bytes and on ONE range of `--big` bytes, device-resident:
                 `--warmup` untimed calls, then the median of `--kernel-reps` device times (alz_last_kernel_ms); next to them the host XXH32 of
                 the single-file layer (alz_framing.h) on one thread over the same bytes.  Every value is checked against the host function.

Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


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
    ap.add_argument("--ranges", type=int, default=10000)
    ap.add_argument("--range-size", type=int, default=262144)
    ap.add_argument("--big", type=int, default=64 << 20)
    ap.add_argument("--kernel-reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd import formats as F
    from auroralib.compression_amd.batch import Context
    result = dict(files=a.files, size=a.size, reps=a.reps)

    def emit(key, value):
        result[key] = value
        print(key, json.dumps(value), flush=True)

    with Context(0) as ctx:
        lib = ctx.lib
        lib.alz_debug_host_xxh32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
        lib.alz_debug_host_xxh32.restype = C.c_uint32
        lib.alz_container_decompress.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]

        def host_xxh32(b):
            return lib.alz_debug_host_xxh32(b, len(b), 0)

        k, n, size = min(a.distinct, a.files), a.files, a.size
        texts = [text_like(size, 100 + i) for i in range(k)]

        def with_content_checksum(frame, content):
            """the frame Compress wrote (FLG 0x40, no checksums) with FLG bit 2 set, the header checksum redone and the content's XXH32 appended"""
            assert frame[:4] == struct.pack("<I", 0x184D2204) and frame[4] == 0x40 and frame[-4:] == bytes(4)
            desc = bytes([frame[4] | 4, frame[5]])
            return frame[:4] + desc + bytes([(host_xxh32(desc) >> 8) & 0xFF]) + frame[7:] + struct.pack("<I", host_xxh32(content))

        sets = (("lz4", A.C_LZ4_FRAME, [with_content_checksum(F.LZ4(BlockSize=0x10000).Compress(t), t) for t in texts]),
                ("snappy", A.C_SNAPPY, [F.Snappy().Compress(t) for t in texts]))
        for name, ct, comps in sets:
            offs, so = [], 0
            for c in comps:
                offs.append(so)
                so += len(c)
            src = np.frombuffer(b"".join(comps) + bytes(1), dtype=np.uint8)
            files = (A.Stream * n)()
            for i in range(n):
                files[i] = A.Stream(offs[i % k], i * size, len(comps[i % k]), size, 0, 0, 0, ct)
            dst = np.empty(n * size, dtype=np.uint8)
            one = np.empty(size, dtype=np.uint8)
            dl, su, st = C.c_size_t(), C.c_size_t(), C.c_int32()

            def batch():
                t = time.perf_counter()
                _, res = ctx.framed_decode_batch(files, src, dst.nbytes, dst=dst)
                w = time.perf_counter() - t
                assert all((r.rc, r.dst_len) == (0, size) for r in res)
                return w

            def loop():
                t = time.perf_counter()
                for i in range(n):
                    c = comps[i % k]
                    rc = lib.alz_container_decompress(ctx.h, ct, None, c, len(c), one.ctypes.data_as(C.c_void_p), size, C.byref(dl), C.byref(su), C.byref(st))
                    assert rc == 0 and dl.value == size
                return time.perf_counter() - t
            batch(), loop()                                                        # warm-up: allocations, code objects
            for i in (0, k - 1, n - 1):
                assert dst[i * size:(i + 1) * size].tobytes() == texts[i % k], i
            assert one.tobytes() == texts[(n - 1) % k]
            tb, tl = [], []
            for _ in range(a.reps):                                                # the two sides alternate
                tb.append(batch())
                tl.append(loop())
            mb, ml = statistics.median(tb), statistics.median(tl)
            emit(name, dict(files=n, compressed_bytes=int(sum(len(comps[i % k]) for i in range(n))),
                            batch_ms=round(mb * 1e3, 2), batch_ms_min=round(min(tb) * 1e3, 2), batch_ms_max=round(max(tb) * 1e3, 2),
                            loop_ms=round(ml * 1e3, 2), loop_ms_min=round(min(tl) * 1e3, 2), loop_ms_max=round(max(tl) * 1e3, 2),
                            loop_over_batch=round(ml / mb, 2), batch_gb_s=round(n * size / 1e9 / mb, 3), loop_gb_s=round(n * size / 1e9 / ml, 3)))

        # XXH32: many ranges, one long range; the bytes are 16 MiB of random data repeated through the buffer
        unit = np.frombuffer(random.Random(7).randbytes(16 << 20), dtype=np.uint8)
        total = max(a.ranges * a.range_size, a.big)
        total = (total + unit.nbytes - 1) // unit.nbytes * unit.nbytes
        d = ctx.malloc(total)
        try:
            for o in range(0, total, unit.nbytes):
                ctx.h2d(C.c_void_p(d.value + o), unit)

            def host_rate(off, ln, count):
                """XXH32 of `count` ranges of ln bytes on one host thread: (value of the first, seconds)"""
                tile = np.concatenate([unit] * ((off % unit.nbytes + ln) // unit.nbytes + 2))[off % unit.nbytes:off % unit.nbytes + ln]
                tile = np.ascontiguousarray(tile)
                t = time.perf_counter()
                for _ in range(count):
                    v = lib.alz_debug_host_xxh32(tile.ctypes.data_as(C.c_void_p), ln, 0)
                return v, time.perf_counter() - t

            def timed(ranges):
                ms = []
                for r in range(a.warmup + a.kernel_reps):
                    got = ctx.xxh32_batch_device(ranges, d, total)
                    if r >= a.warmup:
                        ms.append(ctx.last_kernel_ms())
                return got, statistics.median(ms), min(ms), max(ms)

            many = (A.Stream * a.ranges)()
            for i in range(a.ranges):
                many[i] = A.Stream(i * a.range_size, 0, a.range_size, 0, 0, 0, 0, 0)
            got, med, lo, hi = timed(many)
            per_unit = unit.nbytes // a.range_size if a.range_size <= unit.nbytes and unit.nbytes % a.range_size == 0 else 0
            checks = range(min(a.ranges, max(per_unit, 1)))
            for i in checks:
                assert int(got[i]) == host_rate(i * a.range_size, a.range_size, 1)[0], i
            if per_unit:
                assert all(int(got[i]) == int(got[i % per_unit]) for i in range(a.ranges))
            nbytes = a.ranges * a.range_size
            sample = min(a.ranges, 400)
            _, hs = host_rate(0, a.range_size, sample)
            emit("xxh32_many", dict(ranges=a.ranges, range_size=a.range_size, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                    gb_s=round(nbytes / 1e9 / (med / 1e3), 1), host_one_thread_gb_s=round(sample * a.range_size / 1e9 / hs, 2)))
            big = (A.Stream * 1)(A.Stream(5, 0, a.big - 5, 0, 0, 0, 0, 0))
            got, med, lo, hi = timed(big)
            hv, hs = host_rate(5, a.big - 5, 1)
            assert int(got[0]) == hv
            emit("xxh32_one_range", dict(bytes=a.big - 5, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                                         gb_s=round((a.big - 5) / 1e9 / (med / 1e3), 3), host_one_thread_gb_s=round((a.big - 5) / 1e9 / hs, 2)))
        finally:
            ctx.free(d)
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
