"""usage: python tools/bench_apenc.py [--streams 10000] [--stream-kib 256] [--runs 5] [--shapes synth0,synth8,synth15,bmp0,bmp8,bmp15] [--json OUT]
Device time of aPLib written on an MI355X (alz_apenc_encode_batch_device), per shape, the wavefront emitter (the default) against the lone-lane one
(alz_ctx_set_exact_kernels) on the same build, alternating, `--runs` calls each after a warm-up pair: medians, spreads (max - min), GiB/s of input.
For scale run tools/bench_bitenc.py with the same --shapes in the same session: ALLZ is the nearest relative (tiered sets, a 512 KiB window).

  synth<Q>   `--streams` x `--stream-kib` KiB of the synthetic batch (synthetic LZSS streams decoded on the GPU, as tools/bench_encode.py) at quality Q
  bmp<Q>     `--streams` windows of `--stream-kib` KiB of Test.bmp, spread over the file, at quality Q

Every status is checked, and the first stream of every shape is read back through alz_aplib_decode_batch.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from auroralib.compression_amd import _abi as A  # noqa: E402
from auroralib.compression_amd import synth  # noqa: E402
from auroralib.compression_amd.batch import Context  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=10000)
ap.add_argument("--stream-kib", type=int, default=256)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--shapes", default="synth0,synth8,synth15,bmp0,bmp8,bmp15")
ap.add_argument("--json", default=None)
a = ap.parse_args()
n, size = a.streams, a.stream_kib * 1024
ctx = Context(0)


def synthetic():
    b = synth.make_batch(A.FMT_LZSS, n, size, synth.seed_for(5))
    raw, _ = ctx.decode_batch(b.streams, b.src, b.dst_bytes)
    return raw, synth.stream_records(b.streams)["dst_off"].astype(np.uint64)


def bmp_windows():
    import oracle_lib as O
    data = open(os.path.join(ROOT, "tests", "golden", "Test.lz"), "rb").read()
    bmp, st = O.container_decompress(O.A.C_LZSS, data, lz=O.A.LzProperties.from_bits(10, 6, 2))
    assert st == 0
    bmp = np.frombuffer(bmp, dtype=np.uint8)
    span = len(bmp) - size
    starts = (np.arange(n, dtype=np.int64) * 7919 * 16) % span
    raw = np.empty(n * size + 64, dtype=np.uint8)
    for i, s in enumerate(starts):
        raw[i * size:(i + 1) * size] = bmp[s:s + size]
    return raw, np.arange(n, dtype=np.uint64) * np.uint64(size)


def spread(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 3), "spread_ms": round(max(v) - min(v), 3), "GiB_per_s": round(n * size / 2**30 / (med / 1e3), 2), "runs": [round(x, 3) for x in v]}


out = {"streams": n, "stream_kib": a.stream_kib, "shapes": {}}
raws = {}
cap = int(ctx.lib.alz_apenc_bound(size))
pitch = (cap + 255) // 256 * 256
for shape in a.shapes.split(","):
    src_kind = shape.rstrip("0123456789")
    quality = int(shape[len(src_kind):])
    if src_kind not in raws:
        raws.clear()                                                        # (one raw batch in memory at a time)
        raws[src_kind] = synthetic() if src_kind == "synth" else bmp_windows()
    raw, src_off = raws[src_kind]
    d_src = ctx.malloc(raw.nbytes)
    ctx.h2d(d_src, raw)
    streams = (A.Stream * n)()
    r = synth.stream_records(streams)
    r["src_off"], r["src_len"] = src_off, size
    r["dst_off"] = np.arange(n, dtype=np.uint64) * np.uint64(pitch)
    r["dst_cap"] = cap
    dbytes = n * pitch + 64
    d_dst = ctx.malloc(dbytes)
    times = {0: [], 1: []}
    for run in range(a.runs + 1):                                           # (the first pair is the warm-up)
        for exact in (0, 1):
            ctx.set_exact_kernels(exact)
            try:
                res = ctx.apenc_encode_batch_device(streams, d_src, raw.nbytes, d_dst, dbytes, quality)
            finally:
                ctx.set_exact_kernels(0)
            if run:
                times[exact].append(ctx.last_kernel_ms())
    rr = synth.result_records(res)
    assert (rr["status"] == 0).all() and (rr["src_used"] == size).all(), "an aPLib stream was not written"
    body = ctx.d2h(d_dst, int(rr["dst_len"][0]))
    ds = (A.Stream * 1)(A.Stream(0, 0, len(body), size, 0, 0, 0, 0))
    back, bres = ctx.aplib_decode_batch(ds, np.concatenate([body, np.zeros(64, dtype=np.uint8)]), size + 64)
    o = int(src_off[0])
    assert bres[0].status == 0 and bres[0].dst_len == size and np.array_equal(back[:size], raw[o:o + size]), "aPLib does not read back"
    out["shapes"][shape] = {"wavefront": spread(times[0]), "lone_lane": spread(times[1]), "ratio": round(float(rr["dst_len"].astype(np.int64).sum()) / (n * size), 4)}
    ctx.free(d_dst)
    ctx.free(d_src)
line = json.dumps(out)
print(line)
if a.json:
    open(a.json, "w").write(line + "\n")
