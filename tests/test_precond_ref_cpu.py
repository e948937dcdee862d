"""CPU tests of the preconditioner test infrastructure (tests/precond_ref.py): the factor generator builds the dependency
levels it is asked for, and the long-double restatement of the apply agrees with scipy's triangular solves."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import precond_ref as pr
from conftest import rel_err


@pytest.mark.parametrize("lower", [True, False])
def test_make_factor_levels_and_triangularity(lower):
    levels = [(50, 0), (3, 4), (40, 12, 20), (1, 90), (1, 1), (17, 4, 5), (2, 100)]
    F = pr.make_factor(levels, lower=lower, seed=11)
    N = sum(r for r, _ in [t[:2] for t in levels])
    assert F.shape == (N, N) and sp.isspmatrix_csr(F)
    T = F.tocoo()
    off = T.row != T.col
    assert np.all(T.row[off] > T.col[off]) if lower else np.all(T.row[off] < T.col[off])
    d = F.diagonal()
    assert np.all(np.abs(d) >= 1.0)
    lv = pr.levels_of(F, lower)
    assert np.bincount(lv).tolist() == [t[0] for t in levels]
    # off-diagonal entries per row as requested, moduli summing to <= 0.5 |diagonal|
    offd = np.diff(F.indptr) - 1
    for l, t in enumerate(levels):
        assert np.all(offd[lv == l] == t[1]), l
    s = np.asarray(abs(F - sp.diags(d)).sum(axis=1)).ravel()
    assert np.all(s <= 0.5 * np.abs(d) * (1 + 1e-12))
    # rows are numbered in a random topological order, not level by level
    assert np.any(np.diff(lv if lower else lv[::-1]) < 0)
    # the 40 rows of a level with a window of 20 draw their 12 entries each from the same 20 earlier rows
    r = np.flatnonzero(lv == 2)
    deps = np.concatenate([F.indices[F.indptr[i]:F.indptr[i + 1]] for i in r])
    assert np.unique(deps[~np.isin(deps, r)]).size == 20
    # U is the mirror image of the same recipe
    if not lower:
        Lm = pr.make_factor(levels, lower=True, seed=11)
        assert (abs(Lm[::-1, ::-1] - F) > 0).nnz == 0


def test_make_factor_is_deterministic_and_refuses_impossible_recipes():
    a = pr.make_factor([(10, 0), (5, 3)], seed=4)
    b = pr.make_factor([(10, 0), (5, 3)], seed=4)
    assert (abs(a - b) > 0).nnz == 0
    with pytest.raises(AssertionError):
        pr.make_factor([(3, 0), (1, 5)])              # 5 entries, 3 earlier rows
    with pytest.raises(AssertionError):
        pr.make_factor([(3, 1)])                      # level 0 depends on nothing


def _spsolve_ref(As, L, U, rg, cs, rs, b):
    y = As @ b
    y0 = y[rg] * (1.0 if rs is None else rs[rg])
    z = spla.spsolve_triangular(L.tocsr(), y0, lower=True)
    w = spla.spsolve_triangular(U.tocsr(), z, lower=False)
    out = np.empty_like(w)
    out[cs] = w
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_apply_ref_matches_scipy_triangular_solves(seed):
    rng = np.random.default_rng(seed)
    levels = [(40, 0), (2, 3), (30, 8), (1, 40), (1, 2), (25, 5, 10)]
    L = pr.make_factor(levels, lower=True, seed=seed)
    N = L.shape[0]
    U = pr.make_factor([(N - 30, 0), (30, 6)], lower=False, seed=seed + 9)
    As = (sp.random(N, N, density=4.0 / N, random_state=seed, format="csr") * (1 - 2j) + sp.identity(N)).tocsr()
    rg, cs, rs = rng.permutation(N), rng.permutation(N), rng.uniform(0.5, 2.0, N)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ref = _spsolve_ref(As, L, U, rg, cs, rs, b)
    ld = pr.apply_ref(As, L, U, rg, cs, rs, b)
    assert ld.dtype == np.clongdouble
    assert rel_err(ld.astype(np.complex128), ref) < 1e-13
    f64 = pr.apply_ref(As, L, U, rg, cs, rs, b, np.complex128)
    assert f64.dtype == np.complex128 and rel_err(f64, ref) < 1e-13
    # identity maps and unit scale by None
    assert rel_err(pr.apply_ref(As, L, U, None, None, None, b).astype(np.complex128),
                   _spsolve_ref(As, L, U, np.arange(N), np.arange(N), None, b)) < 1e-13


def test_apply_ref_matches_superlu_of_a_general_matrix():
    # Pr M Pc = L U as the preconditioner wrapper passes it: row_gather / col_scatter are the inverse permutations
    rng = np.random.default_rng(3)
    N = 300
    M = (sp.random(N, N, density=0.03, random_state=5) * (1 + 1j) + sp.diags(rng.uniform(2, 3, N) * np.exp(1j * rng.uniform(0, 6, N)))).tocsc()
    As = (sp.random(N, N, density=0.02, random_state=6) * 1j + sp.identity(N)).tocsr()
    lu = spla.splu(M)
    rg = np.empty(N, np.int64)
    rg[lu.perm_r] = np.arange(N)
    cs = np.empty(N, np.int64)
    cs[lu.perm_c] = np.arange(N)
    b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    ref = lu.solve(As @ b)
    assert rel_err(pr.apply_ref(As, lu.L, lu.U, rg, cs, None, b).astype(np.complex128), ref) < 1e-13


def test_long_double_reference_is_more_accurate_than_double():
    # the f64 baseline of the accuracy criterion is a real baseline: it differs from the long-double result by rounding
    L = pr.make_factor([(200, 0), (100, 30), (50, 60), (1, 300)], lower=True, seed=2)
    U = pr.make_factor([(200, 0), (151, 40)], lower=False, seed=3)
    N = L.shape[0]
    b = np.random.default_rng(1).standard_normal(N) + 0j
    ld = pr.apply_ref(sp.identity(N, format="csr"), L, U, None, None, None, b)
    f64 = pr.apply_ref(sp.identity(N, format="csr"), L, U, None, None, None, b, np.complex128)
    e = float(np.linalg.norm(f64 - ld) / np.linalg.norm(ld))
    assert 0 < e < 1e-14
