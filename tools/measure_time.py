"""usage (GPU box): python tools/measure_time.py [--commit ID] [--streams N] [--bytes B]  -- what a size query costs next to the decode of the same batch.
Device-resident synthetic batches (synth, N x B, default 10 000 x 256 KiB) of PRS BE, LZ4 block, LZO, raw Snappy, FastLZ (lane-parallel measure kernels) and Yaz0
(exact tier, for the record), then two shapes a file produces: 256 x 64 KiB and 16 x 4 MiB LZ4 blocks.  Per batch three warm-ups of each call, then five alternating
pairs of Plan.execute_timed (decode) and Context.measure_batch_device (HIP events around its launches on the same stream: alz_last_kernel_ms); EVERY pair is printed.
The measure call is given no sizes (dst_cap = 0xFFFFFF00, dst_off = 0) and its lengths are checked against the decode's results.
The output of one run is committed as profiles/measure_time.txt."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from auroralib.compression_amd import _abi as A, synth  # noqa: E402
from auroralib.compression_amd.batch import Context, Plan  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def run(ctx, label, fmt, n, size, seed):
    b = synth.make_batch(fmt, n, size, seed)
    d_src, d_dst = ctx.malloc(b.src.nbytes + 64), ctx.malloc(b.dst_bytes + 64)
    ctx.h2d(d_src, b.src)
    wide = (A.Stream * n)()
    rec = synth.stream_records(wide)
    rec[:] = synth.stream_records(b.streams)
    rec["dst_off"], rec["dst_cap"] = 0, A.MEASURE_NO_BOUND
    plan = Plan(ctx, b.streams)
    for _ in range(3):
        plan.execute_timed(d_src, d_dst, iters=1)
        res = ctx.measure_batch_device(wide, d_src, b.src.nbytes)
    want, got = synth.result_records(plan.results()), synth.result_records(res)
    assert (want["status"] == 0).all() and (got["status"] == 0).all() and np.array_equal(want["dst_len"], got["dst_len"]) and np.array_equal(want["src_used"], got["src_used"]), label
    pairs = []
    for _ in range(5):
        dec = plan.execute_timed(d_src, d_dst, iters=1)
        ctx.measure_batch_device(wide, d_src, b.src.nbytes)
        pairs.append((dec, ctx.last_kernel_ms()))
    plan.close()
    ctx.free(d_src)
    ctx.free(d_dst)
    print("%-28s %6d x %8d B (%7.1f MB in, %8.1f MB out): decode / measure ms per pair: %s | measure faster in %d of 5, mean ratio measure / decode %.2f" % (
        label, n, size, b.compressed_bytes / 1e6, b.decompressed_bytes / 1e6, "  ".join("%.3f / %.3f" % p for p in pairs),
        sum(1 for d, m in pairs if m < d), sum(m for _, m in pairs) / sum(d for d, _ in pairs)), flush=True)


def main():
    n, size = int(arg("--streams", "10000")), int(arg("--bytes", "262144"))
    print("# python tools/measure_time.py %s" % " ".join(sys.argv[1:]))
    print("# commit: %s" % arg("--commit", commit_id()))
    with Context(0) as ctx:
        print("# device: %s" % ctx.info()["name"], flush=True)
        for name, fmt in (("prs_be", A.FMT_PRS_BE), ("lz4_block", A.FMT_LZ4_BLOCK), ("lzo", A.FMT_LZO), ("snappy_raw", A.FMT_SNAPPY_RAW), ("fastlz", A.FMT_FASTLZ),
                          ("yaz0 (exact tier)", A.FMT_YAZ0)):
            run(ctx, name, fmt, n, size, synth.seed_for(2))
        run(ctx, "lz4_block, 64 KiB blocks", A.FMT_LZ4_BLOCK, 256, 65536, synth.seed_for(3))
        run(ctx, "lz4_block, 4 MiB blocks", A.FMT_LZ4_BLOCK, 16, 4 << 20, synth.seed_for(4))


if __name__ == "__main__":
    main()
