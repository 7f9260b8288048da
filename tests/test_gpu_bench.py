"""bench.py's own contract, end to end on the GPU at a small batch: a plain run prints the headline line alone, --dump-outputs writes the
last timed step's outputs (float32 / float64 .npy, at most 64 MB) from inputs that are identical run to run, and --full adds the figures
the headline does not need."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "2"] + list(extra),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_bench_plain_run_and_dump_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dumps = []
    for i in range(2):
        d = str(tmp_path / f"out{i}")
        j = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", d)
        assert all(k in j for k in HEADLINE), j
        assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "images/s" and j["higher_is_better"] is True
        assert abs(j["value"] - 2 * 3 / (j["ms_per_step"] * 3e-3)) < 1e-2 * j["value"]
        assert not {"roofline", "encoder_stack", "cpu_baseline", "also"} & set(j), sorted(j)     # the plain run measures the headline alone
        dumps.append(_load(d))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 2 ** 20
    a, b = dumps
    assert {"rec", "q_loss", "loss", "param_sums", "param_sample"} <= set(a) and set(a) == set(b)
    assert a["rec"].shape == (2, 3, 256, 256)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape, k
        assert np.isfinite(a[k]).all(), k
    # same arguments -> same inputs and weights: the two runs agree output for output
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-3, atol=1e-5 * max(1.0, float(np.abs(a[k]).max()))), k


def test_bench_full_adds_the_side_measurements():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    j = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-also")
    assert all(k in j for k in HEADLINE), j
    assert "encoder_stack" in j and j["encoder_stack"]["fwd_ms"] > 0
    assert "roofline" in j and j["roofline"]["launches_timed"] > 0
