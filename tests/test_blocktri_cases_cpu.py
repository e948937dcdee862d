"""CPU tests of the synthetic block-tridiagonal inputs and the long-double sweeps of tests/blocktri_cases.py.

They are what makes the bounds of tests/test_gpu_blocktri_shapes.py meaningful: the inputs need no pivoting, hold no part
in the float-denormal range, and the reference alone stays far inside 1e-12."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import blocktri_ref as bt
import blocktri_cases as bc
from conftest import rel_err

FLOAT_MIN_NORMAL = float(np.finfo(np.float32).tiny)        # 1.18e-38

shapes = pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.shape_id)


def _up_to(limit, size=lambda s: s[0]):
    picked = [s for s in bc.SHAPES if size(s) <= limit]
    return pytest.mark.parametrize("shape", picked, ids=bc.shape_id)


@shapes
def test_generator_shape(shape):
    b, K, pattern = shape
    Msp, As, _ = bc.built(shape)
    N = b * K
    assert Msp.shape == As.shape == (N, N)
    assert np.array_equal(Msp.indptr, As.indptr) and np.array_equal(Msp.indices, As.indices)
    assert Msp.has_sorted_indices and np.all(np.diff(Msp.indptr) >= 1)
    assert bt.in_band(Msp.indptr, Msp.indices, K)
    rows = np.repeat(np.arange(N), np.diff(Msp.indptr))
    on_diag = rows == Msp.indices
    assert on_diag.sum() == N                                                # the diagonal is always stored
    off = np.bincount(rows[~on_diag], weights=np.abs(Msp.data[~on_diag]), minlength=N)
    assert np.all(np.abs(Msp.data[on_diag]) > off)                           # strictly dominant by rows
    kb, cb = rows // b, Msp.indices // b
    if pattern == "blockdiag":
        assert K > 1 and np.all(kb == cb)
    if pattern == "dense":
        assert Msp.nnz == (3 * K - 2) * b * b
    if pattern == "ragged":
        lower, upper = np.bincount(rows[cb < kb], minlength=N), np.bincount(rows[cb > kb], minlength=N)
        inner = np.bincount(rows[cb == kb], minlength=N)
        assert np.sum(lower[b:] == 0) >= (N - b) // 8 and np.sum(upper[:-b] == 0) >= (N - b) // 8
        assert np.sum(inner == 1) >= 1
        if K >= 3:
            k = K // 2
            assert not np.any((kb == k) & (cb == k + 1)) and not np.any((kb == k + 1) & (cb == k))
            assert np.any((kb == k) & (cb == k - 1))                          # the other pair is there
    # the same call gives the same matrices
    again = bc.synth(b, K, pattern, seed=b)
    assert np.array_equal(again[0].data, Msp.data) and np.array_equal(again[1].data, As.data)


@_up_to(257)
def test_no_block_needs_pivoting(shape):
    b, K, _ = shape
    ratio = bc.min_pivot_ratio(bc.built(shape)[0], K)
    print(f"{bc.shape_id(shape)}: smallest |pivot| / max|S_k| = {ratio:.3f}")
    assert ratio >= 1e-3                                   # five orders above the library's breakdown threshold 1e-8


@shapes
def test_no_float_denormals(shape):
    smallest = bc.smallest_part(bc.built(shape)[2])
    print(f"{bc.shape_id(shape)}: smallest non-zero part of any S_k^-1 {smallest:.2e}")
    assert smallest >= FLOAT_MIN_NORMAL


@_up_to(3000, size=lambda s: s[0] * s[1])
def test_long_double_sweeps_match_sparse_lu(shape):
    b, K, _ = shape
    Msp, As, Sinv = bc.built(shape)
    w = As @ bc.right_hand_sides(b * K, 1)[0]
    x = bc.solve_ld(Msp, Sinv, w)
    assert x.dtype == bc.LD and x.shape == w.shape
    xo = spla.splu(Msp.tocsc()).solve(w)
    err, worst = rel_err(x, xo), bc.elementwise_err(x, xo)
    print(f"{bc.shape_id(shape)}: long-double sweeps vs splu {err:.1e} in norm, {worst:.1e} elementwise")
    assert err <= 1e-12 and worst <= 1e-12


def test_sweeps_of_several_members_are_the_single_sweeps():
    shape = (33, 3, "scattered")
    Msp, As, Sinv = bc.built(shape)
    W = (As @ bc.right_hand_sides(99, 3).T).T
    X = bc.solve_ld(Msp, Sinv, W)
    assert X.shape == W.shape
    for j in range(3):
        assert np.array_equal(X[j], bc.solve_ld(Msp, Sinv, W[j]))
    assert rel_err(X[1], bt.solve(Msp, Sinv, W[1])) <= 1e-14
