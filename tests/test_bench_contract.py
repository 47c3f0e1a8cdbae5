"""bench.py is a driver contract: one JSON line on stdout with the
whole-job metric. Pin the schema on CPU (tiny config) so a refactor
can't silently break the round-end measurement."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest


@pytest.mark.timeout(300)
def test_bench_json_contract():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"),
         "--model", "tiny-cpu", "--steps", "2", "--warmup", "1",
         "--batch", "4"],
        env=dict(os.environ, PYTHONPATH=repo), cwd=repo,
        capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout  # exactly ONE JSON line
    rec = json.loads(lines[0])
    assert rec["metric"] == "train tokens/sec (whole node)"
    assert rec["unit"] == "tokens/s"
    assert rec["value"] > 0
    assert rec["n_gpus"] == 1
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert rec["higher_is_better"] is True
    assert rec["scaling"] == "weak"
    assert rec["vs_baseline"] is None
    assert rec["data"] == "synthetic"
    assert math.isfinite(rec["final_loss"])  # trajectory honesty field
    cfg = rec["config"]
    assert set(cfg) >= {"model", "global_batch", "seq_len", "parallelism"}
    assert cfg["parallelism"] == "dp1"
    # whole-job aggregate consistency: value == tokens/step / (ms/1000)
    toks = cfg["global_batch"] * cfg["seq_len"]
    assert abs(rec["value"] - toks / (rec["ms_per_step"] / 1e3)) / rec["value"] < 1e-6


def _bench_dump(repo, out_dir, steps, extra=()):
    out = subprocess.run(
        [sys.executable, os.path.join(repo, "bench.py"),
         "--model", "tiny-cpu", "--steps", str(steps), "--warmup", "1",
         "--batch", "2", "--dump-outputs", str(out_dir), *extra],
        # GPU kernels accumulate with atomics, so only the CPU path is
        # bit-reproducible: hide any GPU from the child
        env=dict(os.environ, PYTHONPATH=repo, HIP_VISIBLE_DEVICES="",
                 CUDA_VISIBLE_DEVICES=""), cwd=repo,
        capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    assert json.loads(lines[0])["dtype"] == "fp32"  # ran on the CPU path
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f))
              for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays


@pytest.mark.timeout(300)
def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed step's loss and updated
    parameters as float32 .npy; same arguments -> same inputs -> (on the
    deterministic CPU path) bit-identical outputs; --steps really sets
    the number of timed steps, so one more step moves the parameters;
    --full is accepted and leaves the headline run as it is."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec_a, a = _bench_dump(repo, tmp_path / "a", 2)
    rec_b, b = _bench_dump(repo, tmp_path / "b", 2, extra=("--full",))
    rec_c, c = _bench_dump(repo, tmp_path / "c", 3)
    assert set(a) == set(b) == set(c) == {"loss", "params"}
    total = 0
    for arr in a.values():
        assert arr.dtype == np.float32
        assert np.isfinite(arr).all()
        total += arr.nbytes
    assert total <= 64 * 1000 * 1000
    assert a["loss"].shape == (1,)
    assert round(float(a["loss"][0]), 4) == rec_a["final_loss"]
    assert set(rec_b) == set(rec_a)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert rec_c["steps"] == 3
    assert not np.array_equal(a["params"], c["params"])
    assert c["loss"][0] != a["loss"][0]
