"""bench.py --dump-outputs: what the last timed step returned, as float32 / float64 .npy files within 64 MB, the same
from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_host_arrays_dtypes():
    bench = _bench()
    got = bench.host_arrays({"pred": torch.ones(3, 2, dtype=torch.bfloat16), "d": torch.zeros(2, dtype=torch.float64),
                             "n": torch.tensor([2 ** 40 + 1]), "loss": torch.tensor(0.5), "note": "not an array"})
    assert set(got) == {"pred", "d", "n", "loss"}
    assert got["pred"].dtype == np.float32 and got["pred"].shape == (3, 2)
    assert got["d"].dtype == np.float64 and got["n"].dtype == np.float64 and got["n"][0] == 2 ** 40 + 1
    assert got["loss"].shape == () and got["loss"] == 0.5


def test_full_is_off_by_default():
    bench = _bench()
    assert bench.parse([]).full is False and bench.parse(["--full"]).full is True


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(5)
    small = {"pred": rng.normal(size=(100, 6, 4)).astype(np.float32), "train/loss": np.float32(1.5)}
    bench.dump_outputs(small, str(tmp_path / "small"))
    assert sorted(os.listdir(tmp_path / "small")) == ["pred.npy", "train_loss.npy"]
    assert np.array_equal(np.load(tmp_path / "small" / "pred.npy"), small["pred"])
    assert np.load(tmp_path / "small" / "train_loss.npy") == np.float32(1.5)
    # past the budget every array keeps the same seeded rows: parameters and gradients stay aligned, runs agree
    params = np.arange(40000, dtype=np.float32)
    big = {"params": params, "grads": -params, "loss": np.float32(2.0)}
    for run in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / run), budget=100000)
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 100000
    p, g = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    assert 0 < len(p) < len(params) and np.array_equal(g, -p) and np.all(np.diff(p) > 0)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def _run_bench(args, out_dir, **env_vars):
    env = dict(os.environ, **env_vars)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out_dir)]
                       + args, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')][-1])
    files = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    assert files and all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir)) <= 64 * 10 ** 6
    return line, files


@pytest.mark.gpu
def test_bench_dump_outputs(tmp_path):
    """Forward mode twice with the same arguments: the same `pred` (same scenes, weights and order draws); train mode:
    the loss of the last timed step and a sample of the parameters and gradients after it."""
    fwd = ["--steps", "3", "--warmup", "1", "--points", "20000", "--no-extra", "--cpu-sample", "0",
           "--no-kernel-events"]
    line, a = _run_bench(fwd, tmp_path / "a")
    _, b = _run_bench(fwd, tmp_path / "b")
    assert line["steps"] == 3 and sorted(a) == ["pred"]
    assert a["pred"].shape == (20000, 6, 4) and np.isfinite(a["pred"]).all()
    assert ((a["pred"][..., 3] >= 0) & (a["pred"][..., 3] <= 1)).all()
    assert np.abs(a["pred"] - b["pred"]).max() <= 1e-3
    line, t = _run_bench(["--mode", "train", "--steps", "2", "--warmup", "1", "--points", "20000",
                          "--no-kernel-events"], tmp_path / "t")
    assert {"loss", "params", "grads"} <= set(t) and t["loss"].shape == ()
    assert float(t["loss"]) == pytest.approx(line["final_loss"], rel=1e-6)
    assert 0 < len(t["params"]) == len(t["grads"]) < 46181592      # sampled: the whole model is past 64 MB
    assert np.isfinite(t["params"]).all() and np.isfinite(t["grads"]).all() and np.abs(t["grads"]).max() > 0


@pytest.mark.gpu
def test_plain_run_times_and_dumps_what_full_run_does(tmp_path):
    """A plain run reports the headline alone; --full adds the rest.  Both time the same forwards: the plain run makes
    the order-shuffle draws of the parity leg it skips, so the two dump the same `pred`."""
    args = ["--steps", "3", "--warmup", "1", "--points", "20000", "--cpu-sample", "100000", "--no-extra",
            "--no-kernel-events"]
    plain, a = _run_bench(args, tmp_path / "plain", PTV3_BENCH_CPU_REPS="1")
    full, b = _run_bench(args + ["--full"], tmp_path / "full", PTV3_BENCH_CPU_REPS="1")
    assert plain["full"] is False and full["full"] is True
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["latency_ms_median"] > 0
    for key in ("throughput_2_in_flight", "cpu_baseline", "parity", "fp32", "roofline", "other_workloads"):
        assert plain[key] is None, key
    assert full["throughput_2_in_flight"]["value"] > 0 and full["cpu_baseline"]["value"] > 0
    assert full["parity"]["fp32"]["offset_l2_max"] < 1e-4
    assert sorted(a) == sorted(b) == ["pred"]
    assert np.abs(a["pred"] - b["pred"]).max() <= 1e-3
