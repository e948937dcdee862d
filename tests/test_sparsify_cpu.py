"""CPU tests of the sparsifying-matrix assembly: the host pattern entry (lsfc_sparsify_pattern) against the restatement
of the reference (tests/sparsify_ref.py), its argument checks, and the restatement itself against the dense G."""
import ctypes as C

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import sparsify_ref as ref


@pytest.mark.parametrize("dims", [(5, 5, 1), (21, 21, 1), (21, 9, 1), (3, 3, 3), (8, 8, 8), (15, 10, 9)])
def test_pattern_matches_the_reference(dims):
    import fast_solver_lippmann_schwinger_amd as pkg
    rowptr, col, cls = pkg.sparsify_pattern(*dims)
    r_ptr, r_col, r_cls, r_nnz = ref.pattern(*dims)
    assert col.size == r_nnz
    assert np.array_equal(rowptr, r_ptr)
    assert np.array_equal(col, r_col)
    assert np.array_equal(cls, r_cls) and cls.min() == 0


def test_pattern_rejects_unsupported_grids():
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    nnz = C.c_int64(-7)
    for dims in [(4, 5, 1), (5, 4, 1), (2, 5, 1), (5, 2, 1), (5, 5, 2), (2, 8, 8), (8, 8, 2)]:
        rc = lib.lsfc_sparsify_pattern(*dims, C.byref(nnz), None, None, None)
        assert rc == -1, dims
        assert b"sparsify" in lib.lsfc_last_error(), dims
    assert lib.lsfc_sparsify_pattern(5, 5, 1, None, None, None, None) == -1
    assert lib.lsfc_sparsify_pattern(5, 7, 1, C.byref(nnz), None, None, None) == 0
    assert nnz.value == (3 * 5 - 2) * (3 * 7 - 2)


def _direct_case(n):
    h = 1.0 / (n - 1)
    x = np.linspace(0.0, 1.0, n)
    X, Y = o.grid2d(x, x)
    k = 1.0 / h
    D0 = o.reference_vals_trap_rule()[1][0]                 # D0 = D[1], examples/example.jl:45
    return X, Y, h, k, D0


def test_restatement_sparsifies_the_dense_kernel():
    n = 21
    X, Y, h, k, D0 = _direct_case(n)
    G = o.build_conv_matrix(k, X, Y, D0, h)
    out = ref.build(ref.direct_rows(k, X, Y, D0, h), n, n)
    As = out["As"].tocsr()
    AsG = As @ G
    for c, (sA, ind, _, _) in enumerate(out["classes"]):
        # the row placed at the sample point carries exactly the sample stencil: its far field is sigma_min
        r = int(sA[0] - 1 - ind[0])
        S = np.asarray(sA) - 1
        assert np.array_equal(np.sort(As[r].indices), np.sort(S)), c
        far = np.setdiff1d(np.arange(n * n), S)
        assert abs(np.linalg.norm(AsG[r, far]) - out["sigma"][c, 2]) <= 1e-12 * out["sigma"][c, 2], c
    # interior rows: the far field of As G is a few sigma_min / sigma_max of the row of G (Ying 2014)
    smin, smax = out["sigma"][0, 2], out["sigma"][0, 0]
    worst = 0.0
    for i, j in [(3, 3), (10, 10), (5, 15), (17, 2), (1, 1), (19, 19)]:
        r = i + n * j
        near = [(i + a) + n * (j + b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
        far = np.setdiff1d(np.arange(n * n), near)
        worst = max(worst, np.linalg.norm(AsG[r, far]) / np.linalg.norm(G[r]))
    assert worst <= 10 * smin / smax, (worst, smin / smax)
