"""usage (GPU box): python tools/rlh_time.py [--commit ID] [--streams N] [--bytes B] [--distinct D]  -- the two kernel families of the RLE30 / HUF20 entry points side by side.
The bytes are those a synthetic LZ10 batch (synth, N x B, default 10 000 x 64 KiB) decodes to, on the device:
  RLE30    every buffer compressed by alz_rlh_encode_batch_device (its kernel time is printed too), then decoded;
  RLHudson the same through alz_rlhudson_encode_batch_device / alz_rlhudson_decode_batch_device (RLE30's kernels over another grammar);
  HUF20-8  / HUF20-4 (little nibble order) of the same bytes.  HUF20 has no encoder, so the streams are assembled on the host: the tree of tests/rlh_ref.py
           (huf20_tree, test-only) per buffer, the code words packed with numpy.  That costs seconds per thousand buffers, so D (default 1 000) distinct
           buffers are built and laid out N / D times -- N separate copies in HBM: the traffic is that of N streams, the content repeats.
Device-resident, three warm-ups of either family, then FIVE INTERLEAVED PAIRS production / exact (alz_ctx_set_exact_kernels; HIP events around the call's
launches: alz_last_kernel_ms); every pair is printed, with GiB/s of decoded bytes.  Outputs and results of both families are compared with the bytes that
went in.  As a scale only, the unchanged LZ10 plan over the batch the bytes came from is timed in the same run.
Decision rule per format: the production kernel stays the default only if it is faster in all five pairs (docs/EXPERIMENTS.md).
The output of one run is committed as profiles/rlh_time.txt."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import rlh_ref as R  # noqa: E402  (the test-only HUF20 tree builder)
from auroralib.compression_amd import _abi as A, synth  # noqa: E402
from auroralib.compression_amd.batch import Context, Plan  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def huf_stream(raw, bits):
    """one HUF20 body for `raw` (np.uint8), or None when the label layout overflows"""
    syms = raw if bits == 8 else np.stack([raw & 15, raw >> 4], axis=1).ravel()      # little order: the low nibble is the even symbol (HUF20.cs:145)
    freq = np.bincount(syms, minlength=1 << bits)
    tree = R.huf20_tree({int(s): int(f) for s, f in enumerate(freq) if f}, bits)
    if tree is None:
        return None
    code, ln = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.int64)
    for s, (c, l) in tree[1].items():
        code[s], ln[s] = c, l
    assert ln.max() <= 32
    l, c = ln[syms], code[syms]
    end = np.cumsum(l)
    off = end - l
    nw = (int(end[-1]) + 31) >> 5
    w = off >> 5
    val = c << (64 - (off & 31) - l).astype(np.uint64)                               # the code inside the 64-bit window that starts at its first word
    starts = np.flatnonzero(np.r_[True, w[1:] != w[:-1]])
    words = np.zeros(nw + 1, dtype=np.uint64)
    words[w[starts]] += np.add.reduceat(val >> np.uint64(32), starts)                # (codes do not overlap: the sum is the OR)
    words[w[starts] + 1] += np.add.reduceat(val & np.uint64(0xFFFFFFFF), starts)
    return tree[0] + words[:nw].astype("<u4").tobytes()


def timed_pairs(ctx, call):
    for _ in range(3):
        for exact in (0, 1):
            ctx.set_exact_kernels(exact)
            call()
    pairs = []
    for _ in range(5):
        ms = []
        for exact in (0, 1):
            ctx.set_exact_kernels(exact)
            call()
            ms.append(ctx.last_kernel_ms())
        pairs.append(tuple(ms))
    ctx.set_exact_kernels(0)
    return pairs


def report(label, n, size, in_bytes, pairs):
    out = n * size
    wins = sum(1 for p, e in pairs if p < e)
    mp, me = sum(p for p, _ in pairs) / 5, sum(e for _, e in pairs) / 5
    print("%-10s %6d x %7d B (%7.1f MB in, %7.1f MB out): production / exact ms per pair: %s | production faster in %d of 5; mean %.3f ms = %.1f GiB/s / %.3f ms = %.1f GiB/s -> default: %s" % (
        label, n, size, in_bytes / 1e6, out / 1e6, "  ".join("%.3f / %.3f" % p for p in pairs), wins, mp, out / 2**30 / (mp / 1e3), me, out / 2**30 / (me / 1e3),
        "production" if wins == 5 else "exact"), flush=True)


def decode_case(ctx, label, fmt, streams, d_src, src_bytes, dst_bytes, raw, doffs, size, check_n, decode=None):
    """fmt None: RLHudson (`decode` is its entry point); the managed encoder's defect is RLE30's"""
    decode = decode or ctx.rlh_decode_batch_device
    n = len(streams)
    d_dst = ctx.malloc(dst_bytes + 64)
    try:
        both = []
        for exact in (1, 0):                                                       # both families: results and bytes
            ctx.set_exact_kernels(exact)
            ctx.memset(d_dst, 0, dst_bytes)
            res = synth.result_records(decode(streams, d_src, src_bytes, d_dst, dst_bytes)).copy()
            ok = (res["status"] == 0) & (res["dst_len"] == size)
            # (RLE30 only: a buffer whose last token is the managed encoder's 129-literal run does not decode back -- DESIGN.md 1, E7)
            assert ok.all() or fmt in (A.RLH_RLE30, None), (label, exact, np.unique(res["status"], return_counts=True))
            for i in list(range(check_n)) + [n - 1]:
                if ok[i]:
                    assert np.array_equal(ctx.d2h(d_dst, size, int(doffs[i])), raw[i]), (label, exact, i)
            both.append(res)
        assert all(np.array_equal(both[0][k], both[1][k]) for k in ("status", "dst_len", "src_used")), label
        if not ok.all():
            print("# %s: %d of %d buffers end in the encoder's over-long literal run and do not decode back (both families agree on them)" % (label, int((~ok).sum()), n))
        pairs = timed_pairs(ctx, lambda: decode(streams, d_src, src_bytes, d_dst, dst_bytes))
        report(label, n, size, int(synth.stream_records(streams)["src_len"].astype(np.int64).sum()), pairs)
    finally:
        ctx.free(d_dst)


def main():
    n, size, distinct = int(arg("--streams", "10000")), int(arg("--bytes", "65536")), int(arg("--distinct", "1000"))
    distinct = min(distinct, n)
    print("# python tools/rlh_time.py %s" % " ".join(sys.argv[1:]))
    print("# commit: %s" % arg("--commit", commit_id()))
    with Context(0) as ctx:
        print("# device: %s" % ctx.info()["name"], flush=True)
        # the bytes: a synthetic LZ10 batch, decoded on the device (and the scale: the unchanged LZ10 plan)
        b = synth.make_batch(A.FMT_LZ10, n, size, synth.seed_for(2))
        d_lz, d_raw = ctx.malloc(b.src.nbytes + 64), ctx.malloc(b.dst_bytes + 64)
        ctx.h2d(d_lz, b.src)
        plan = Plan(ctx, b.streams)
        for _ in range(3):
            plan.execute_timed(d_lz, d_raw, iters=1)
        lz = [plan.execute_timed(d_lz, d_raw, iters=1) for _ in range(5)]
        assert (synth.result_records(plan.results())["status"] == 0).all()
        plan.close()
        ctx.free(d_lz)
        doffs = synth.stream_records(b.streams)["dst_off"].copy()
        print("%-10s %6d x %7d B (%7.1f MB in, %7.1f MB out): the LZ10 plan over the batch these bytes come from, ms per execute: %s | mean %.3f ms = %.1f GiB/s (scale only)" % (
            "lz10", n, size, b.compressed_bytes / 1e6, n * size / 1e6, "  ".join("%.3f" % v for v in lz), sum(lz) / 5, n * size / 2**30 / (sum(lz) / 5e3)), flush=True)
        raw = [ctx.d2h(d_raw, size, int(doffs[i])) for i in range(distinct)] + [None] * (n - distinct)
        raw[n - 1] = ctx.d2h(d_raw, size, int(doffs[n - 1]))

        # ---- RLE30: compressed on the device, then decoded
        slot = (2 * size + 8 + 255) // 256 * 256
        enc = (A.Stream * n)()
        rec = synth.stream_records(enc)
        rec["src_off"], rec["src_len"], rec["dst_off"], rec["dst_cap"], rec["format"] = doffs, size, np.arange(n, dtype=np.uint64) * slot, slot, A.RLH_RLE30
        d_rle = ctx.malloc(n * slot + 64)
        eres = synth.result_records(ctx.rlh_encode_batch_device(enc, d_raw, b.dst_bytes, d_rle, n * slot))
        assert (eres["status"] == 0).all()
        ems = []
        for _ in range(5):
            ctx.rlh_encode_batch_device(enc, d_raw, b.dst_bytes, d_rle, n * slot)
            ems.append(ctx.last_kernel_ms())
        print("%-10s %6d x %7d B (%7.1f MB in, %7.1f MB out): RLE30 ENCODE (one kernel for both families), ms per call: %s | mean %.3f ms = %.1f GiB/s of raw bytes" % (
            "rle30 enc", n, size, n * size / 1e6, int(eres["dst_len"].astype(np.int64).sum()) / 1e6, "  ".join("%.3f" % v for v in ems), sum(ems) / 5, n * size / 2**30 / (sum(ems) / 5e3)), flush=True)
        dec = (A.Stream * n)()
        rec = synth.stream_records(dec)
        rec["src_off"], rec["src_len"], rec["dst_off"], rec["dst_cap"], rec["decom_len"], rec["format"] = np.arange(n, dtype=np.uint64) * slot, eres["dst_len"], doffs, size, size, A.RLH_RLE30
        decode_case(ctx, "rle30", A.RLH_RLE30, dec, d_rle, n * slot, b.dst_bytes, raw, doffs, size, min(distinct, 16))
        # ---- RLHudson, RLE30's sibling (the same kernels over another grammar): the same buffers, compressed on the device, then decoded
        rec = synth.stream_records(enc)
        rec["format"] = 0
        eres = synth.result_records(ctx.rlhudson_encode_batch_device(enc, d_raw, b.dst_bytes, d_rle, n * slot))
        assert (eres["status"] == 0).all()
        ems = []
        for _ in range(5):
            ctx.rlhudson_encode_batch_device(enc, d_raw, b.dst_bytes, d_rle, n * slot)
            ems.append(ctx.last_kernel_ms())
        print("%-10s %6d x %7d B (%7.1f MB in, %7.1f MB out): RLHudson ENCODE (one kernel for both families), ms per call: %s | mean %.3f ms = %.1f GiB/s of raw bytes" % (
            "rlhud enc", n, size, n * size / 1e6, int(eres["dst_len"].astype(np.int64).sum()) / 1e6, "  ".join("%.3f" % v for v in ems), sum(ems) / 5, n * size / 2**30 / (sum(ems) / 5e3)), flush=True)
        rec = synth.stream_records(dec)
        rec["src_len"], rec["format"] = eres["dst_len"], 0
        decode_case(ctx, "rlhudson", None, dec, d_rle, n * slot, b.dst_bytes, raw, doffs, size, min(distinct, 16), decode=ctx.rlhudson_decode_batch_device)
        ctx.free(d_rle)
        ctx.free(d_raw)

        # ---- HUF20: streams assembled on the host
        for label, fmt, bits in (("huf20_8", A.RLH_HUF20_8, 8), ("huf20_4", A.RLH_HUF20_4, 4)):
            bodies, owner = [], []                                                   # body i decodes to raw[owner[i]]
            for i in range(distinct):
                s = huf_stream(raw[i], bits)
                if s is None and not bodies:
                    raise SystemExit("%s: the first buffer overflows the 6-bit tree offsets" % label)
                bodies.append(s if s is not None else bodies[-1])
                owner.append(i if s is not None else owner[-1])
            skipped = sum(1 for i, o in enumerate(owner) if o != i)
            if skipped:
                print("# %s: %d of %d distinct buffers overflow the 6-bit tree offsets and repeat their neighbour" % (label, skipped, distinct))
            hslot = (max(len(s) for s in bodies) + 15) // 16 * 16
            blob = np.zeros((distinct, hslot), dtype=np.uint8)
            for i, s in enumerate(bodies):
                blob[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
            reps = (n + distinct - 1) // distinct
            src = np.concatenate([np.tile(blob, (reps, 1))[:n].ravel(), np.zeros(64, dtype=np.uint8)])
            st = (A.Stream * n)()
            rec = synth.stream_records(st)
            lens = np.array([len(s) for s in bodies], dtype=np.uint32)
            rec["src_off"], rec["src_len"] = np.arange(n, dtype=np.uint64) * hslot, np.tile(lens, reps)[:n]
            rec["dst_off"], rec["dst_cap"], rec["decom_len"], rec["format"] = doffs, size, size, fmt
            want = [raw[owner[i % distinct]] for i in range(n)]
            d_src = ctx.malloc(src.nbytes + 64)
            ctx.h2d(d_src, src)
            decode_case(ctx, label, fmt, st, d_src, src.nbytes - 64, b.dst_bytes, want, doffs, size, min(distinct, 16))
            ctx.free(d_src)


if __name__ == "__main__":
    main()
