"""A plain bench.py run: exactly the steps asked for, the headline fields, nothing of --full, and --dump-outputs of the
last timed step -- the same inputs in two runs with the same arguments, so the same outputs up to the summation order
of the kernels' float atomics."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_and_dumps_the_last_step(tmp_path):
    line, err = _plain_run(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(32 / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert line["metric"] == "clip-query pairs/sec (fwd+bwd)" and line["unit"] == "pairs/s" and line["higher_is_better"]
    assert line["config"]["full"] is False and line["cpu_baseline"] is None and line["roofline"]["achieved"] is None
    assert line["config"]["settled_not_in_metric"] is None and line["config"]["unchanged_caller_not_in_metric"] is None
    assert "settled:" not in err and "cpu baseline" not in err
    files = sorted(os.listdir(tmp_path / "a"))
    assert "loss.npy" in files and "grad.npy" in files and np.load(tmp_path / "a" / "grad.npy").size > 10 ** 7
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10 ** 6
    for f in files:
        a = np.load(tmp_path / "a" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
    _plain_run(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == files
    # other draws or dropout masks would differ at O(1).  What the bounds leave room for is the run-to-run freedom of the
    # default arithmetic: the float atomics' summation order, which now and then also flips a PReLU kink within rounding
    # of zero (measured: 1.2e-4 of the gradient's largest element, relative L2 5e-5; loss entries within 1e-7) -- the
    # bound of test_model_gpu.py::test_run_to_run_spread_of_a_replayed_step
    for f in files:
        a, b = np.load(tmp_path / "a" / f).astype(np.float64), np.load(tmp_path / "b" / f).astype(np.float64)
        if f.startswith("loss"):
            assert float(np.abs(a - b).max()) < 1e-6 * max(1.0, float(np.abs(a).max())), f
        else:
            assert float(np.abs(a - b).max()) <= 1e-3 * float(np.abs(a).max()), f
            assert float(np.linalg.norm(a - b)) < 1e-3 * float(np.linalg.norm(a)), f
