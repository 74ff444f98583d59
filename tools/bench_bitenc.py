"""usage: python tools/bench_bitenc.py [--streams 10000] [--stream-kib 256] [--runs 5] [--shapes synth0,synth8,bmp8] [--json OUT]
Device time of CRILAYLA and ALLZ written on an MI355X (alz_bitenc_encode_batch_device), per kind and shape, the wavefront emitters (the default)
against the lone-lane ones (alz_ctx_set_exact_kernels) on the same build, alternating, `--runs` calls each: medians and spreads (max - min).
Yaz0 through alz_encode_batch_device on the same batch in the same run is the yardstick for the finder's share: the same kernels A and B at an
8 KiB / 4 KiB window, a parse + emit kernel that is known to be cheap.

  synth0 / synth8   `--streams` x `--stream-kib` KiB of the synthetic batch (synthetic LZSS streams decoded on the GPU, as tools/bench_encode.py) at quality 0 / 8
  bmp8              `--streams` windows of `--stream-kib` KiB of Test.bmp, spread over the file, at quality 8

Every status is checked, and the first stream of every (kind, shape) is read back through alz_bitlz_decode_batch.  Prints one JSON line."""
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
ap.add_argument("--shapes", default="synth0,synth8,bmp8")
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


def table(kind_or_fmt, src_off, cap, aux0=0):
    streams = (A.Stream * n)()
    r = synth.stream_records(streams)
    r["src_off"], r["src_len"] = src_off, size
    pitch = (cap + 255) // 256 * 256
    r["dst_off"] = np.arange(n, dtype=np.uint64) * np.uint64(pitch)
    r["dst_cap"], r["format"], r["aux0"] = cap, kind_or_fmt, aux0
    return streams, n * pitch + 64


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "spread_ms": round(max(v) - min(v), 3), "runs": [round(x, 3) for x in v]}


out = {"streams": n, "stream_kib": a.stream_kib, "shapes": {}}
raws = {}
for shape in a.shapes.split(","):
    src_kind = shape.rstrip("0123456789")
    quality = int(shape[len(src_kind):])
    if src_kind not in raws:
        raws.clear()                                                        # (one raw batch in memory at a time)
        raws[src_kind] = synthetic() if src_kind == "synth" else bmp_windows()
    raw, src_off = raws[src_kind]
    d_src = ctx.malloc(raw.nbytes)
    ctx.h2d(d_src, raw)
    row = {}
    # the yardstick: Yaz0 on the same batch
    ys, ybytes = table(A.FMT_YAZ0, src_off, size + size // 4 + 64)
    d_dst = ctx.malloc(ybytes)
    ms = []
    for _ in range(a.runs + 1):
        res, _aux = ctx.encode_batch_device(ys, d_src, raw.nbytes, d_dst, ybytes, quality=quality)
        ms.append(ctx.last_kernel_ms())
    assert (synth.result_records(res)["status"] == 0).all()
    row["yaz0"] = spread(ms[1:])
    ctx.free(d_dst)
    for kind in (A.BITLZ_CRILAYLA, A.BITLZ_ALLZ):
        cap = ctx.lib.alz_bitenc_bound(kind, size) if kind == A.BITLZ_CRILAYLA else size + size // 4 + 1024
        streams, dbytes = table(kind, src_off, cap, A.allz_aux0() if kind == A.BITLZ_ALLZ else 0)
        d_dst = ctx.malloc(dbytes)
        times = {0: [], 1: []}
        for run in range(a.runs + 1):                                       # (the first pair is the warm-up)
            for exact in (0, 1):
                ctx.set_exact_kernels(exact)
                try:
                    res = ctx.bitenc_encode_batch_device(streams, d_src, raw.nbytes, d_dst, dbytes, quality)
                finally:
                    ctx.set_exact_kernels(0)
                if run:
                    times[exact].append(ctx.last_kernel_ms())
        rr = synth.result_records(res)
        assert (rr["status"] == 0).all(), "a %s stream did not fit its slot" % A.BITLZ_NAMES[kind]
        body = ctx.d2h(d_dst, int(rr["dst_len"][0]))
        ds = (A.Stream * 1)(A.Stream(0, 0, len(body), size, size, A.allz_aux0(), 0, kind))
        back, bres = ctx.bitlz_decode_batch(ds, np.concatenate([body, np.zeros(64, dtype=np.uint8)]), size + 64)
        o = int(src_off[0])
        assert bres[0].status == 0 and np.array_equal(back[:size], raw[o:o + size]), "%s does not read back" % A.BITLZ_NAMES[kind]
        row[A.BITLZ_NAMES[kind]] = {"wavefront": spread(times[0]), "lone_lane": spread(times[1]), "ratio": round(float(rr["dst_len"].astype(np.int64).sum()) / (n * size), 4)}
        ctx.free(d_dst)
    ctx.free(d_src)
    out["shapes"][shape] = row
line = json.dumps(out)
print(line)
if a.json:
    open(a.json, "w").write(line + "\n")
