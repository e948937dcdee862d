"""CPU tests of the GMRES test infrastructure (tests/gmres_ref.py): the long-double restatement agrees with oracle.gmres
in double, its grouped form equals the same problem on full vectors, and the recipes reach the paths they are meant to."""
import numpy as np
import pytest

import gmres_ref as gr
from oracle import lsfc_oracle as o

_ORACLE = {"MGS": "ModifiedGramSchmidt", "CGS": "ClassicalGramSchmidt", "DGKS": "DGKS"}


def _live_rel(h, ref):
    """< 1e-10 stands for history_excess < 1: 1e-10 relative, plus the restart allowance"""
    return gr.history_excess(h, ref)[0] * 1e-10


@pytest.mark.parametrize("orth", gr.ORTHS)
@pytest.mark.parametrize("restart", [1, 3, 30, 70])
def test_reference_matches_oracle_in_double(orth, restart):
    N = 500
    lam, b = gr.disc_spectrum(N, 0.9, seed=restart), gr.random_rhs(N, seed=7)
    ref = gr.gmres_ref(b, pl=lam, restart=restart, maxiter=130, orth=orth)
    x = np.zeros(N, complex)
    x, h = o.gmres(x, lambda v: v.copy(), b, Pl=lambda v: lam * v, restart=restart, maxiter=130, orth_meth=_ORACLE[orth])
    assert (h.iters, h.mvps, h.isconverged) == (ref["iters"], ref["mvps"], ref["converged"])
    assert _live_rel(h.resnorm, ref) < 1e-10
    assert np.linalg.norm(x - ref["x"].astype(complex)) / np.linalg.norm(x) < 1e-10
    # the same GMRES with the operator as A instead of Pl
    x2 = np.zeros(N, complex)
    x2, h2 = o.gmres(x2, lambda v: lam * v, lam * b, restart=restart, maxiter=130, orth_meth=_ORACLE[orth])
    ref2 = gr.gmres_ref(lam * b, a=lam, restart=restart, maxiter=130, orth=orth)
    assert (h2.iters, h2.mvps) == (ref2["iters"], ref2["mvps"]) and _live_rel(h2.resnorm, ref2) < 1e-10


@pytest.mark.parametrize("orth", gr.ORTHS)
def test_reference_initially_zero_abstol_and_start_vector(orth):
    N = 300
    lam, b = gr.disc_spectrum(N, 0.8, seed=2), gr.random_rhs(N, seed=3)
    x0 = 0.1 * gr.random_rhs(N, seed=4)
    ref = gr.gmres_ref(b, pl=lam, restart=9, maxiter=200, reltol=0.0, abstol=1e-6, orth=orth, x0=x0)
    x = x0.copy()
    x, h = o.gmres(x, lambda v: v.copy(), b, Pl=lambda v: lam * v, restart=9, maxiter=200, reltol=0.0, abstol=1e-6,
                   orth_meth=_ORACLE[orth])
    assert (h.iters, h.mvps, h.isconverged) == (ref["iters"], ref["mvps"], True) and _live_rel(h.resnorm, ref) < 1e-10
    z = gr.gmres_ref(b, pl=lam, restart=9, maxiter=40, orth=orth, initially_zero=True)
    x = np.zeros(N, complex)
    x, h = o.gmres(x, lambda v: v.copy(), b, Pl=lambda v: lam * v, restart=9, maxiter=40, orth_meth=_ORACLE[orth],
                   initially_zero=True)
    assert (h.iters, h.mvps) == (z["iters"], z["mvps"]) == (40, 1 + 40 + 4) and _live_rel(h.resnorm, z) < 1e-10


@pytest.mark.parametrize("orth", gr.ORTHS)
def test_grouped_form_equals_full_vectors(orth):
    N, m = 1500, 37
    g = gr.group_map(N, m)
    c = gr.group_counts(g, m)
    assert c.sum() == N and c.min() >= N // m and c.max() <= N // m + 1
    # every block of 64 consecutive entries and the tail hold several groups
    assert all(np.unique(g[i:i + 64]).size > 8 for i in range(0, N, 64))
    lam, b = gr.disc_spectrum(m, 0.9, seed=5), gr.random_rhs(m, seed=6)
    grp = gr.gmres_ref(b, pl=lam, counts=c, restart=12, maxiter=30, orth=orth)
    full = gr.gmres_ref(b[g], pl=lam[g], restart=12, maxiter=30, orth=orth)
    assert (grp["iters"], grp["mvps"], grp["converged"]) == (full["iters"], full["mvps"], full["converged"])
    assert np.max(np.abs(grp["resnorm_ld"] - full["resnorm_ld"]) / full["resnorm_ld"]) < 1e-15
    assert np.max(np.abs(grp["x"][g] - full["x"])) / np.max(np.abs(full["x"])) < 1e-15
    assert grp["passes"] == full["passes"]


def test_dgks_recipe_reorthogonalises_and_disc_recipe_stays_above_tolerance():
    N = 2000
    lam, b = gr.cluster_spectrum(N, 1e-3, seed=1), gr.random_rhs(N, seed=2)
    ref = gr.gmres_ref(b, pl=lam, restart=30, maxiter=30, orth="DGKS")
    assert sum(ref["passes"]) >= 1 and max(ref["passes"]) < 8
    lam, b = gr.disc_spectrum(N, 0.9, seed=1), gr.random_rhs(N, seed=2)
    for restart in (30, 100):
        ref = gr.gmres_ref(b, pl=lam, restart=restart, maxiter=100, orth="MGS")
        assert not ref["converged"] and ref["iters"] == 100
        assert ref["resnorm"][-1] > 10 * gr.DEFAULT_RELTOL * ref["beta0"]


@pytest.mark.parametrize("kind", ["small-N1", "small-N2", "small-N3", "small-N5", "unit", "identity", "seven"])
@pytest.mark.parametrize("orth", gr.ORTHS)
def test_exhausted_krylov_space_converges(kind, orth):
    N, m, lam, b, restart = gr.exhausted_problem(kind)
    counts = None if m is None else gr.group_counts(gr.group_map(N, m), m)
    ref = gr.gmres_ref(b, pl=lam, counts=counts, restart=restart, orth=orth)
    dim = len(b) if m is None else m
    assert ref["converged"] and 1 <= ref["iters"] <= dim
    assert np.all(np.isfinite(ref["x"]))
    # diag(lam) x = diag(lam) b: the solution is b
    assert np.max(np.abs(ref["x"] - b)) / np.max(np.abs(b)) < 1e-12


def test_oracle_converges_on_an_exact_zero_subdiagonal():
    # N = 5, A = I: the first Arnoldi step leaves w == 0 exactly; the reference treats that as convergence, as the oracle
    # does through abs(inf + nan im)**2 == inf
    b = gr.random_rhs(5, seed=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        x, h = o.gmres(np.zeros(5, complex), lambda v: v.copy(), b)
    ref = gr.gmres_ref(b)
    assert h.isconverged and ref["converged"] and h.iters == ref["iters"] == 1
    assert ref["subdiag"][0] == 0 and h.resnorm[0] == 0 and ref["resnorm"][0] == 0
    assert np.allclose(x, b, rtol=0, atol=1e-15) and np.allclose(ref["x"].astype(complex), b, rtol=0, atol=1e-15)
