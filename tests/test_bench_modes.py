"""bench.py: a plain run does only what its headline figure needs, --full adds the parity gate, the per-stage roofline and
the CPU baseline; the contrast it builds a few planes at a time on threads is bitwise the whole-volume sum (CPU), and
the two kinds of run print what they should (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from cases import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _nu_whole_volume(n, lo, hi):
    """the contrast as one whole-volume expression per Gaussian"""
    rng = np.random.default_rng(1234)
    cen = rng.uniform(-0.3, 0.3, size=(8, 3))
    amp = rng.uniform(-0.3, 0.3, size=8)
    beta = rng.uniform(20, 80, size=8)
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    z = x[lo:hi]
    out = np.zeros((hi - lo, n, n))
    for c, a, b in zip(cen, amp, beta):
        gx = np.exp(-b * (x - c[0]) ** 2)
        gy = np.exp(-b * (x - c[1]) ** 2)
        gz = np.exp(-b * (z - c[2]) ** 2)
        out += a * gz[:, None, None] * gy[None, :, None] * gx[None, None, :]
    return out.reshape(-1)


@pytest.mark.parametrize("n,lo,hi", [(40, 0, 40), (64, 16, 48), (128, 0, 128), (384, 100, 109), (512, 505, 512), (100, 3, 3)])
def test_synthetic_nu_is_bitwise_the_whole_volume_sum(n, lo, hi):
    a, b = bench.synthetic_nu(n, lo, hi), _nu_whole_volume(n, lo, hi)
    assert a.shape == b.shape == ((hi - lo) * n * n,)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_full_is_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert (a.full, a.no_cpu_baseline, a.no_parity_gate, a.dump_outputs) == (False, False, False, None)
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1)
    assert bench.parse_args(["--full"]).full
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def _line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", "64", "--steps", "3", "--warmup", "1", *args],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_and_full_lines(lsfc):
    plain = _line()
    assert all(k in plain for k in HEADLINE) and plain["value"] > 0 and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["unit"] == "applies/s" and plain["dtype"] == "f64" and plain["higher_is_better"] is True
    assert plain["parity_rel_l2"] == "gate not run (run with --full)"
    assert "roofline" not in plain and "cpu_baseline" not in plain

    full = _line("--full")
    assert all(k in full for k in HEADLINE) and full["value"] > 0
    assert set(full["parity_rel_l2"]) == {"n64", "n128"} and max(full["parity_rel_l2"].values()) <= full["parity_tol"] <= TOL
    stages = [s["kernel"] for s in full["roofline"]["stages"]]
    assert stages[0] == "xfwd" and stages[-1] == "xinv" and full["roofline"]["kernel"] in stages
    assert full["cpu_baseline"]["value"] > 0 and full["gpu_over_cpu"] > 0

    skipped = _line("--full", "--no-parity-gate", "--no-cpu-baseline")
    assert skipped["parity_rel_l2"] == "gate skipped (--no-parity-gate)" and "cpu_baseline" not in skipped and "roofline" in skipped
