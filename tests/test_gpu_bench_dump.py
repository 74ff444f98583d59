"""-m gpu: a plain bench.py run -- set-up, warm-up, exactly --steps timed steps and the line, nothing else -- and what --dump-outputs
writes: the last timed step's outputs (per-stream results, a CRC-32 of every stream's bytes, the bytes of a seeded sample of streams),
checked here against the CPU restatement of the same seeded batch, stream by stream."""
import json
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(launch, out_dir, *extra):
    """bench.py without --full, started by the session's clean launcher (tests/conftest.py); returns (contract line, dumped arrays)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--dump-outputs", str(out_dir)] + list(extra)
    rc, out, err = launch(cmd, env=dict(os.environ), cwd=ROOT, timeout=600)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert rc == 0 and len(lines) == 1 and out.splitlines()[-1] == lines[0], (rc, out[-2000:], err[-3000:])
    d = json.loads(lines[0])
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "u8"
    # a plain run measures nothing beyond the headline figure
    assert d["cpu_baseline"] is None and "configs_summary" not in d and "end_to_end" not in d and "copy_bandwidth" not in d
    files = sorted(os.listdir(out_dir))
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    arrays = {f[:-len(".npy")]: np.load(os.path.join(out_dir, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    return d, arrays


def test_plain_decode_run_dumps_what_the_last_step_decoded(clean_launcher, tmp_path):
    import oracle_lib as O
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd import synth
    from auroralib.compression_amd.sharding import shard_seed
    n, target = 256, 65536
    d, o = _plain_run(clean_launcher, tmp_path / "decode", "--streams", str(n), "--stream-kib", "64", "--steps", "3")
    assert d["steps"] == 3 and d["unit"] == "GiB/s" and d["config"]["format"] == "yaz0"
    assert d["config"]["parity_ok"] is True and d["config"]["verified_vs_oracle"] is None and "pipelined" not in d["config"]
    assert set(o) == {"status", "dst_len", "src_used", "decoded_crc32", "sample_streams", "decoded_sample"}
    b = synth.make_batch(np.full(n, A.FORMAT_NAMES.index("yaz0"), dtype=np.uint32), n, target, shard_seed(2, 0, n))   # bench.py's batch
    dst, res = O.decode_batch(b.streams, b.src, b.dst_bytes, nthreads=4)
    rr, recs = synth.result_records(res), synth.stream_records(b.streams)
    assert (rr["status"] == 0).all() and (rr["dst_len"] == target).all()
    for k in ("status", "dst_len", "src_used"):
        assert np.array_equal(o[k], rr[k].astype(np.float64)), k
    offs = recs["dst_off"].astype(np.int64)
    assert o["decoded_crc32"].tolist() == [zlib.crc32(dst[a:a + target].tobytes()) for a in offs]
    pick = o["sample_streams"].astype(np.int64)
    assert o["decoded_sample"].shape == (len(pick), target) and len(pick) > 0 and len(set(pick.tolist())) == len(pick)
    for r, i in enumerate(pick):
        assert np.array_equal(o["decoded_sample"][r], dst[offs[i]:offs[i] + target].astype(np.float32)), i


def test_plain_encode_run_dumps_what_the_last_step_compressed(clean_launcher, tmp_path):
    import oracle_lib as O
    from auroralib.compression_amd import _abi as A
    from auroralib.compression_amd import synth
    from auroralib.compression_amd.sharding import shard_seed
    n, target, q = 32, 65536, 8
    d, o = _plain_run(clean_launcher, tmp_path / "encode", "--mode", "encode", "--streams", str(n), "--stream-kib", "64", "--quality", str(q),
                      "--steps", "2")
    assert d["steps"] == 2 and d["config"]["mode"] == "encode" and d["config"]["format"] == "lzss"
    assert d["config"]["parity_ok"] is True and d["config"]["verified_roundtrip_and_vs_oracle"] is None
    assert set(o) == {"status", "dst_len", "aux", "compressed_crc32", "sample_streams", "compressed_sample"}
    b = synth.make_batch(A.FMT_LZSS, n, target, shard_seed(5, 0, n))                     # bench.py's raw buffers: these streams, decoded
    raw, _ = O.decode_batch(b.streams, b.src, b.dst_bytes, nthreads=4)
    offs = synth.stream_records(b.streams)["dst_off"].astype(np.int64)
    want = [O.encode_stream(A.FMT_LZSS, raw[a:a + target].tobytes(), quality=q) for a in offs]
    assert (o["status"] == 0).all()
    assert o["dst_len"].tolist() == [len(w) for w, _ in want]
    assert o["compressed_crc32"].tolist() == [zlib.crc32(w) for w, _ in want]
    assert o["aux"].tolist() == [[x.aux0, x.aux1] for _, x in want]
    pick = o["sample_streams"].astype(np.int64)
    assert len(pick) > 0
    for r, i in enumerate(pick):
        w = np.frombuffer(want[i][0], dtype=np.uint8)
        row = o["compressed_sample"][r]
        assert np.array_equal(row[:len(w)], w.astype(np.float32)) and not row[len(w):].any(), i
