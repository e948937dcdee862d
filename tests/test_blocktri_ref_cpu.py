"""CPU tests of the block-tridiagonal elimination of Msp: the numpy restatement (tests/blocktri_ref.py) against
scipy's sparse LU, and the band structure of the pattern lsfc_sparsify_pattern returns.

Bound 1e-10: the project's parity bar for the preconditioner (tests/test_gpu_precond.py); the
restatement is observed at <= 1.0e-14."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import lsfc_oracle as o
import blocktri_ref as bt
from conftest import rel_err

CASES = [("trap", (41, 41, 1)), ("trap", (101, 101, 1)), ("gv3", (16, 16, 16)), ("gv3", (18, 12, 10)), ("gv3", (24, 24, 24))]


@pytest.mark.parametrize("kind,dims", CASES)
def test_elimination_matches_sparse_lu(kind, dims):
    Msp, As = bt.ref_pair(kind, dims)
    K = dims[1] if dims[2] == 1 else dims[2]
    assert bt.in_band(Msp.indptr, Msp.indices, K) and bt.in_band(As.indptr, As.indices, K)
    Sinv = bt.eliminate(Msp, K)
    v = o.random_vector(Msp.shape[0])
    w = As @ v
    x = bt.solve(Msp, Sinv, w)
    xo = spla.splu(Msp.tocsc()).solve(w)
    err, res = rel_err(x, xo), float(np.linalg.norm(Msp @ x - w) / np.linalg.norm(w))
    cond = max(np.linalg.cond(np.linalg.inv(S)) for S in Sinv[:: max(1, K // 4)])
    print(f"{kind} {dims}: b = {Msp.shape[0] // K}, cond(S_k) <= {cond:.0f}, difference to splu {err:.1e}, residual {res:.1e}")
    assert err <= 1e-10 and res <= 1e-10


@pytest.mark.parametrize("kind,dims", [("trap", (41, 41, 1)), ("gv3", (16, 16, 16))])
def test_schur_blocks_invert_without_pivoting(kind, dims):
    # the device inversion does not pivot: the restatement's Schur blocks must not need it
    Msp, _ = bt.ref_pair(kind, dims)
    K = dims[1] if dims[2] == 1 else dims[2]
    worst_diff, worst_pivot = 0.0, np.inf
    for Si in bt.eliminate(Msp, K):
        G, ratio = bt.gauss_jordan_nopivot(np.linalg.inv(Si))
        worst_diff, worst_pivot = max(worst_diff, rel_err(G, Si)), min(worst_pivot, ratio)
    print(f"{kind} {dims}: pivot-free inverse within {worst_diff:.1e}, smallest |pivot| / max|S_k| = {worst_pivot:.2f}")
    assert worst_diff <= 1e-10 and worst_pivot >= 1e-2        # six orders above the library's breakdown threshold 1e-8


@pytest.mark.parametrize("dims", [(41, 41, 1), (101, 101, 1), (33, 33, 1), (16, 16, 16), (18, 12, 10), (24, 24, 24)])
def test_pattern_lies_inside_the_three_block_diagonals(dims):
    import fast_solver_lippmann_schwinger_amd as pkg
    rowptr, col, _ = pkg.sparsify_pattern(*dims)
    K = dims[1] if dims[2] == 1 else dims[2]
    assert bt.in_band(rowptr, col, K)
    assert not bt.in_band(rowptr, col, dims[0] * K)          # a finer split is not block tridiagonal: the check can fail
