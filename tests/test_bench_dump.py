"""bench.py --dump-outputs: the sample of y it writes is fixed and bounded (CPU), and what it writes at n = 64 is the
operator apply of the bench's own inputs (GPU, against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from cases import TOL
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_sample_is_fixed_and_bounded():
    assert np.array_equal(bench.dump_indices(64 ** 3), np.arange(64 ** 3))
    N = 512 ** 3
    idx = bench.dump_indices(N)
    assert np.array_equal(idx, bench.dump_indices(N))
    assert idx.size == bench.DUMP_POINTS and idx.size * 16 <= 64 * 2 ** 20
    assert idx[0] >= 0 and idx[-1] < N and np.all(np.diff(idx) > 0)


def test_gather_points_over_slabs_and_write(tmp_path):
    N = 40 ** 3
    y = torch.from_numpy(np.random.default_rng(3).standard_normal(2 * N).view(np.complex128))
    idx = np.sort(np.random.default_rng(4).choice(N, 5000, replace=False))
    cuts = [0, 7 * 1600, 31 * 1600, N]
    parts = [bench.gather_points(idx, [(lo, y[lo:hi])]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert torch.equal(sum(parts), y[torch.from_numpy(idx)])
    assert torch.equal(bench.gather_points(idx, [(lo, y[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]), y[torch.from_numpy(idx)])
    bench.write_outputs(str(tmp_path / "d"), y.numpy())
    a = np.load(tmp_path / "d" / "y.npy")
    assert a.dtype == np.float64 and a.shape == (N, 2)
    assert np.array_equal(a[:, 0] + 1j * a[:, 1], y.numpy())


@pytest.mark.gpu
def test_bench_dump_outputs_match_oracle(lsfc, tmp_path):
    from oracle import lsfc_oracle as o
    n = 64
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", str(n), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    a = np.load(tmp_path / "y.npy")
    assert a.dtype == np.float64 and a.shape == (n ** 3, 2)
    h = 1.0 / n
    G2 = o.reduced_symbol_gv3d(n, n, n, n * h, 1.0 / h, patch_singular=False)
    ref = o.apply_reduced(G2, bench.synthetic_nu(n, 0, n), 1.0 / h, bench.bench_vector(n, 0, n), (n, n, n))
    assert rel_err(a[:, 0] + 1j * a[:, 1], ref) < TOL
