"""`bench.py --dump-outputs DIR`: after the timed steps the last step's outputs land in DIR as float
.npy files (at most 64 MB), `--steps` sets the number of timed steps, and two runs with the same
arguments start from the same inputs and so compute the same outputs (up to reduction-order rounding)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--repeats", "1", "--crop", "64x128", "--no-check", "--no-cpu-baseline", "--no-k3-timer",
           "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_bench_dump_outputs(tmp_path):
    runs = [_bench(tmp_path / "a"), _bench(tmp_path / "b")]
    for d in runs:
        assert d["steps"] == 3 and len(d["config"]["archs"]) == 3
        assert d["ms_per_step"] > 0 and d["config"]["passes"]["repeats"] == 1
    a, b = tmp_path / "a", tmp_path / "b"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"loss.npy", "params.npy", "momentum.npy", "bn_running.npy"} <= set(names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all()
        scale = max(float(np.abs(y).max()), 1e-6)
        assert float(np.abs(x.astype(np.float64) - y).max()) <= 1e-4 * scale, n
    assert np.load(a / "params.npy").shape == (1 << 22,)
    assert abs(float(np.load(a / "loss.npy")) - runs[0]["config"]["last_loss"]) < 1e-4


def _bench_args(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + [str(a) for a in args]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def test_bench_full_adds_fields_only(tmp_path):
    """A plain run leaves out what `--full` adds (the first step's oracle comparison, the K3 roofline
    pass, roofline_step, the CPU baseline); `--full` adds those fields after the same steps, so both
    runs time the same draws and dump the same outputs."""
    common = ["--steps", 3, "--warmup", 1, "--repeats", 1, "--crop", "64x128"]
    plain = _bench_args(common + ["--dump-outputs", tmp_path / "plain"])
    full = _bench_args(common + ["--full", "--cpu-baseline-size", "64x128",
                                 "--dump-outputs", tmp_path / "full"])
    assert not {"roofline", "roofline_step", "cpu_baseline"} & set(plain)
    assert plain["check"]["status"] == "skipped" and "--full" in plain["check"]["reason"]
    assert {"roofline", "roofline_step", "cpu_baseline"} <= set(full)
    assert full["roofline"]["launches"] > 0 and full["roofline_step"]["achieved"] > 0
    assert full["cpu_baseline"]["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["ms_per_step"] > 0 and full["ms_per_step"] > 0
    assert plain["config"]["archs"] == full["config"]["archs"]
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    for n in names:
        x, y = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert x.shape == y.shape
        scale = max(float(np.abs(y).max()), 1e-6)
        assert float(np.abs(x.astype(np.float64) - y).max()) <= 1e-4 * scale, n
