"""usage: python tools/bench_bitlz.py [--streams 10000] [--size 262144] [--reps 12] [--warmup 3] [--formats crilayla,allz] [--skip-single] [--json OUT]
Device time of CRILAYLA and ALLZ decode (alz_bitlz_decode_batch_device) on an MI355X, per format:

  batch   `--streams` streams that decode to `--size` bytes each, built from 32 distinct token-level generated streams, repeated.
          CRILAYLA: 30 % literals, else a match of 3 + Exp(10) bytes at a log-uniform distance in [3, min(produced, 8194)].
          ALLZ (copy, dist, len = 0, 10, 1): every second match is preceded by a run of 1 + Exp(4) random bytes; matches of 3 + Exp(10) bytes
          at a log-uniform distance in [1, min(produced, 65535)].
  single  one stream of 1 000 KiB through the host form (alz_bitlz_decode_batch: upload, decode, download), wall clock and device time --
          the shape of the reference's Benchmarks.md rows (Decompress of 1 000 KiB: CRILAYLA 2 380 / 1 884 us, ALLZ 4 774 / 3 924 us)

Protocol: `--warmup` untimed calls, then the median of `--reps` (>= 12) device times (HIP events around the launch, alz_last_kernel_ms); every
stream's status, dst_len and src_used are checked against the generator's own count, the first 4 KiB of every distinct stream against the
restatement (tests/bitlz_ref.py).  Prints one JSON line."""
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

import bitlz_ref as R  # noqa: E402

PARAMS = (0, 10, 1)


def log_uniform(rng, lo, hi):
    return max(lo, min(hi, int(math.exp(rng.uniform(math.log(lo), math.log(hi + 1))))))


def gen_crilayla(rng, size):
    """(body, decoded size, token counts); the bit strings of bitlz_ref.cri_token_bits, written with format() for speed"""
    parts, produced, counts = [], 0, dict(lit=0, match=0)
    while produced < size:
        room = size - produced
        if produced < 3 or room < 3 or rng.random() < 0.30:
            parts.append("0" + format(rng.randrange(256), "08b")); produced += 1; counts["lit"] += 1
            continue
        d = log_uniform(rng, 3, min(produced, 8194))
        L = min(3 + int(rng.expovariate(1 / 10.0)), room)
        s = "1" + format(d - 3, "013b")
        rem, vle = L - 3, 0
        while rem >= R.VLE_FLAGS[vle]:
            s += format(R.VLE_FLAGS[vle], "0%db" % R.VLE_LEVELS[vle]); rem -= R.VLE_FLAGS[vle]; vle = min(vle + 1, 3)
        parts.append(s + format(rem, "0%db" % R.VLE_LEVELS[vle])); produced += L; counts["match"] += 1
    bits = "".join(parts)
    bits += "0" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "little"), produced, counts    # (first bit = top bit of the LAST byte)


def gen_allz(rng, size):
    """(body, decoded size, token counts) through bitlz_ref.AllzWriter"""
    w, produced, counts = R.AllzWriter(), 0, dict(run=0, match=0)
    copy, dist, ln = PARAMS
    after_run, want_run = False, True
    while produced < size:
        room = size - produced
        if want_run or room < 3:
            n = min(1 + int(rng.expovariate(1 / 4.0)), room)
            if room - n < 3:
                n = room                                                         # (a run may end the stream; a match of fewer than 3 bytes cannot)
            w.bit(0); w.alflag(ln, n - 1); w.raw(bytes(rng.randrange(256) for _ in range(n)))
            produced += n; counts["run"] += 1; after_run = True; want_run = False
            continue
        if not after_run:
            w.bit(1)
        d = log_uniform(rng, 1, min(produced, 65535))
        L = min(3 + int(rng.expovariate(1 / 10.0)), room)
        w.alflag(dist, d - 1); w.alflag(copy, L - 3)
        produced += L; counts["match"] += 1
        want_run, after_run = not after_run, False                               # every second match has a run in front
    return w.bytes(), produced, counts


GEN = {"crilayla": gen_crilayla, "allz": gen_allz}


def build_batch(fmt, distinct, size, seed):
    rng = random.Random(seed)
    uniq = [GEN[fmt](rng, size) for _ in range(distinct)]
    offs, so, chunks = [], 0, []
    for u in uniq:
        offs.append(so)
        chunks.append(u[0] + bytes((-len(u[0])) % 256))
        so += len(chunks[-1])
    src = np.frombuffer(b"".join(chunks) + bytes(64), dtype=np.uint8).copy()
    return uniq, offs, src, {k: sum(u[2][k] for u in uniq) for k in uniq[0][2]}


def first_4k(fmt, body, size):
    """the restatement's first 4 KiB of output, in memory order (CRILAYLA: the TOP 4 KiB of the span)"""
    n = min(4096, size)
    return R.cri_decode(body, n)[0] if fmt == "crilayla" else R.allz_decode(body, size, n, *PARAMS)[0]


def time_batch(ctx, A, fmt, uniq, offs, src, n, size, reps, warmup):
    kind = A.BITLZ_CRILAYLA if fmt == "crilayla" else A.BITLZ_ALLZ
    cap = (size + 255) // 256 * 256
    streams = (A.Stream * n)()
    for i in range(n):
        u = i % len(uniq)
        streams[i] = A.Stream(offs[u], i * cap, len(uniq[u][0]), size, size, A.allz_aux0(*PARAMS), 0, kind)
    dst_bytes = n * cap + 64
    modes = (("exact", 0),)                                                      # (one kernel per format; kernels built both ways would alternate here)
    d_src, d_dst = ctx.malloc(src.nbytes), ctx.malloc(dst_bytes)
    out, ms, first = {}, {m: [] for m, _ in modes}, {}
    try:
        ctx.h2d(d_src, src)
        ctx.memset(d_dst, 0xA5, dst_bytes)
        for r in range(warmup + reps):
            for mode, variant in modes:                                          # alternating
                ctx.set_kernel_variant(variant)
                res = ctx.bitlz_decode_batch_device(streams, d_src, src.nbytes, d_dst, dst_bytes)
                if r >= warmup:
                    ms[mode].append(ctx.last_kernel_ms())
                if r in (0, warmup + reps - 1):
                    for i in range(n):
                        u = uniq[i % len(uniq)]
                        assert (res[i].status, res[i].dst_len, res[i].src_used) == (0, u[1], len(u[0])), (mode, i, res[i].status, res[i].dst_len, res[i].src_used)
                if r == 0:
                    for u in range(min(len(uniq), n)):
                        got = ctx.d2h(d_dst, size, offset=u * cap)
                        if u not in first:
                            first[u] = got
                            want = first_4k(fmt, uniq[u][0], size)
                            part = got[size - len(want):] if fmt == "crilayla" else got[:len(want)]
                            assert part.tobytes() == want, (mode, u)
                        else:
                            assert np.array_equal(got, first[u]), (mode, u)
        for mode, _ in modes:
            med = statistics.median(ms[mode])
            out[mode] = dict(ms=round(med, 3), ms_min=round(min(ms[mode]), 3), ms_max=round(max(ms[mode]), 3), gib_s=round(n * size / 2**30 / (med / 1e3), 2))
    finally:
        ctx.set_kernel_variant(0)
        ctx.free(d_src)
        ctx.free(d_dst)
    out["in_bytes_per_stream"] = int(sum(len(u[0]) for u in uniq) / len(uniq))
    return out


def time_single(ctx, A, fmt, reps, warmup):
    body, n, _ = GEN[fmt](random.Random(357), 1000 << 10)
    kind = A.BITLZ_CRILAYLA if fmt == "crilayla" else A.BITLZ_ALLZ
    st = (A.Stream * 1)(A.Stream(0, 0, len(body), n, n, A.allz_aux0(*PARAMS), 0, kind))
    buf = np.frombuffer(body + bytes(64), dtype=np.uint8).copy()
    wall, dev = [], []
    for r in range(warmup + reps):
        t = time.perf_counter()
        dst, res = ctx.bitlz_decode_batch(st, buf, n + 64)
        w = time.perf_counter() - t
        if r >= warmup:
            wall.append(w * 1e3); dev.append(ctx.last_kernel_ms())
    assert (res[0].status, res[0].dst_len, res[0].src_used) == (0, n, len(body))
    want = first_4k(fmt, body, n)
    assert (dst[n - len(want):n] if fmt == "crilayla" else dst[:len(want)]).tobytes() == want
    return dict(wall_ms=round(statistics.median(wall), 3), kernel_ms=round(statistics.median(dev), 3),
                kernel_gib_s=round(n / 2**30 / (statistics.median(dev) / 1e3), 3), in_bytes=len(body))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=10000)
    ap.add_argument("--size", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--formats", default="crilayla,allz")
    ap.add_argument("--skip-single", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert a.reps >= 12 or a.streams < 100, "the protocol wants the median of at least 12"
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd.batch import Context
    result = dict(streams=a.streams, size=a.size, reps=a.reps)
    with Context(0) as ctx:
        for fmt in a.formats.split(","):
            t0 = time.time()
            uniq, offs, src, counts = build_batch(fmt, a.distinct, a.size, 355)
            r = dict(tokens=counts, gen_s=round(time.time() - t0, 1))
            r["batch"] = time_batch(ctx, A, fmt, uniq, offs, src, a.streams, a.size, a.reps, a.warmup)
            print(fmt, "batch", json.dumps(r["batch"]), flush=True)
            if not a.skip_single:
                r["single_1000KiB"] = time_single(ctx, A, fmt, a.reps, a.warmup)
                print(fmt, "single", json.dumps(r["single_1000KiB"]), flush=True)
            result[fmt] = r
    line = json.dumps(result)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
