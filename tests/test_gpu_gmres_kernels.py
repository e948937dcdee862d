"""GPU tests of the device GMRES kernels (csrc/gmres.hip, csrc/krylov_blas.hip) against the long-double restatement of
tests/gmres_ref.py, at the vector lengths, restart lengths and path switches where a Krylov kernel goes wrong.

The operator: a plan with a finite symbol and nu == 0, so that M * x == x bitwise, and the left preconditioner
diag(lambda) -- the device SparsifyingPreconditioner with Msp = I, As = diag(lambda) (identity LU factors passed in, no
splu), or a host / torch callback.  GMRES then iterates on exactly diag(lambda), and equal entries stay bitwise equal on
the device: only the reductions see the order of summation.  Histories must match the reference to 1e-10 relative (plus
the restart allowance of gmres_ref.history_excess) while it is above 1e-9 beta, x to 1e-10."""
import functools

import numpy as np
import pytest

import gmres_ref as gr
import krylov_common as kc
from krylov_common import _diag_precond, plan  # noqa: F401  (plan: the cached identity plans)

pytestmark = pytest.mark.gpu

ORTH = {"MGS": "ModifiedGramSchmidt", "CGS": "ClassicalGramSchmidt", "DGKS": "DGKS"}
# (orth, LSFC_MGS_BLOCK) of the device paths: strict / blocked MGS, fused or chunked CGS, DGKS
PATHS = [("MGS", "0"), ("MGS", "1"), ("CGS", None), ("DGKS", None)]
LARGE = [1 << 20, (1 << 20) + 3, (1 << 22) - 1, 1 << 22, (1 << 22) + 1]   # 2^20 + 1 = 17 * 61681 has no plan shape


_REFS = {}


def _ref(key, b, lam, counts=None, **kw):
    if key not in _REFS:
        _REFS[key] = gr.gmres_ref(b, pl=lam, counts=counts, **kw)
    return _REFS[key]


_check = functools.partial(kc._check, history_excess=gr.history_excess)


def _solve(lsfc, M, P, b, monkeypatch, orth, mgs_block=None, lookahead=None, **kw):
    for name, val in (("LSFC_MGS_BLOCK", mgs_block), ("LSFC_GMRES_LOOKAHEAD", lookahead)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    x = np.zeros(M.N, complex)
    return lsfc.gmres_(x, M, b, Pl=P, log=True, orth_meth=ORTH[orth], **kw)


# -- vector lengths: reduction tails and block boundaries, every path, lookahead off and on --------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4095, 65538])
def test_vector_lengths(lsfc, plan, monkeypatch, N):
    M = plan(N)
    lam, b = gr.disc_spectrum(N, 0.9, seed=N), gr.random_rhs(N, seed=N + 1)
    P = _diag_precond(lsfc, lam)
    try:
        for orth, mb in PATHS:
            ref = _ref(("len", N, orth), b, lam, restart=30, maxiter=100, orth=orth)
            out = {}
            for la in ("0", "1"):
                x, h = _solve(lsfc, M, P, b, monkeypatch, orth, mb, la, restart=30, maxiter=100)
                _check(f"N={N} {orth} block={mb} lookahead={la}", x, h, ref)
                out[la] = (x, h)
            # the lookahead changes when kernels are posted, not what they compute
            (x0, h0), (x1, h1) = out["0"], out["1"]
            assert np.array_equal(h0["resnorm"], h1["resnorm"]) and np.array_equal(x0, x1), f"N={N} {orth} block={mb}"
    finally:
        P.close()


# -- restart lengths: blocked-MGS remainders, the fused / chunked CGS boundary at 64 / 65, the chunked x += V y -------
@pytest.mark.parametrize("N,restart", [(N, r) for N in (1025, 4097) for r in (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 100)]
                         + [(65, 100)])
def test_restart_lengths(lsfc, plan, monkeypatch, N, restart):
    M = plan(N)
    lam, b = gr.disc_spectrum(N, 0.9, seed=N), gr.random_rhs(N, seed=N + 1)
    P = _diag_precond(lsfc, lam)
    maxiter = 100 if restart < 100 else 130
    try:
        for orth, mb in [("MGS", "1"), ("MGS", "0"), ("CGS", None)] + ([("DGKS", None)] if restart in (64, 65) else []):
            if restart >= 63 and (orth, mb) == ("MGS", "0"):
                continue
            ref = _ref(("restart", N, restart, orth), b, lam, restart=restart, maxiter=maxiter, orth=orth)
            x, h = _solve(lsfc, M, P, b, monkeypatch, orth, mb, restart=restart, maxiter=maxiter)
            _check(f"N={N} restart={restart} {orth} block={mb}", x, h, ref)
    finally:
        P.close()


# -- large N on the natural path: the 1024-block cap of the reductions, the 2^22 switches ----------------------------
@pytest.mark.parametrize("N", LARGE)
@pytest.mark.parametrize("orth", ["MGS", "CGS"])
def test_large_grouped(lsfc, plan, monkeypatch, N, orth):
    m = 331
    gmap = gr.group_map(N, m)
    counts = gr.group_counts(gmap, m)
    # (a faster rate, 0.6, makes classical Gram-Schmidt itself lose orthogonality by the end of a 30-step cycle: the
    # double-precision reference then strays from the long-double one as far as the device does)
    lam_g, b_g = gr.disc_spectrum(m, 0.8, seed=3), gr.random_rhs(m, seed=4)
    ref = _ref(("large", N, orth), b_g, lam_g, counts=counts, restart=30, maxiter=200, orth=orth)
    M = plan(N)
    P = _diag_precond(lsfc, lam_g[gmap])
    try:
        x, h = _solve(lsfc, M, P, b_g[gmap], monkeypatch, orth, restart=30, maxiter=200)
    finally:
        P.close()
    label = f"N={N} {orth}"
    # every group bitwise constant: an element that a tail skipped or updated twice breaks it
    first = np.zeros(m, dtype=np.int64)
    first[gmap[::-1]] = np.arange(N - 1, -1, -1)
    bad = np.flatnonzero(np.any(x.view(np.float64).reshape(-1, 2) != x[first][gmap].view(np.float64).reshape(-1, 2), axis=1))
    assert bad.size == 0, f"{label}: x is not constant on its groups: first index {bad[0]} (group {gmap[bad[0]]}), " \
                          f"{bad.size} entries differ"
    assert h.isconverged and ref["iters"] > 60                       # two restarts, then convergence
    _check(label, x, h, ref, gmap)


# -- bitwise equalities ----------------------------------------------------------------------------------------------
def test_repeated_solves_are_bitwise_equal(lsfc, plan, monkeypatch):
    N = 4097
    M = plan(N)
    lam, b = gr.disc_spectrum(N, 0.9, seed=1), gr.random_rhs(N, seed=2)
    P = _diag_precond(lsfc, lam)
    try:
        for orth, mb in PATHS:
            x0, h0 = _solve(lsfc, M, P, b, monkeypatch, orth, mb, restart=20, maxiter=50)
            x1, h1 = _solve(lsfc, M, P, b, monkeypatch, orth, mb, restart=20, maxiter=50)
            assert np.array_equal(h0["resnorm"], h1["resnorm"]) and np.array_equal(x0, x1), (orth, mb)
    finally:
        P.close()


def test_batch_equals_single_solves_bitwise(lsfc, plan, monkeypatch):
    # three right-hand sides that converge at different iterations, one host callback, batched vs one by one
    monkeypatch.delenv("LSFC_GMRES_LOOKAHEAD", raising=False)
    N = 4097
    M = plan(N)
    lam = gr.disc_spectrum(N, 0.6, seed=5)
    B = np.zeros((3, N), complex)
    B[0] = gr.random_rhs(N, seed=6)
    B[1, :12] = gr.random_rhs(12, seed=7)               # 12 eigen-components: converges within 12 steps
    B[2, 100:140] = gr.random_rhs(40, seed=8)

    def Pl(v):
        v *= lam

    for orth in ("MGS", "CGS", "DGKS"):
        X = np.zeros((3, N), complex)
        X, hb = lsfc.gmres_batch_(X, M, B, Pl=Pl, restart=20, log=True, orth_meth=ORTH[orth])
        its = [hh.iters for hh in hb]
        assert len(set(its)) == 3 and all(hh.isconverged for hh in hb), its
        for j in range(3):
            x = np.zeros(N, complex)
            x, h = lsfc.gmres_(x, M, B[j], Pl=Pl, restart=20, log=True, orth_meth=ORTH[orth])
            assert (h.iters, h.mvps) == (hb[j].iters, hb[j].mvps), (orth, j)
            assert np.array_equal(h["resnorm"], hb[j]["resnorm"]) and np.array_equal(x, X[j]), (orth, j)
            # zero entries of b stay zero: the reference on the support alone (default restart and maxiter of N)
            nz = B[j] != 0
            ref = gr.gmres_ref(B[j][nz], pl=lam[nz], counts=None, restart=20, maxiter=N, orth=orth)
            assert np.all(x[~nz] == 0), (orth, j)
            _check(f"batch {orth} rhs {j}", x[nz], h, ref)


# -- other routes to the same operator -------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "torch"])
def test_callback_routes(lsfc, plan, monkeypatch, route):
    import torch
    N = 1025
    M = plan(N)
    lam, b = gr.disc_spectrum(N, 0.9, seed=N), gr.random_rhs(N, seed=N + 1)
    lam_t = torch.from_numpy(lam).cuda()
    calls = []

    def host(v):
        calls.append(v.size)
        v *= lam

    def dev(v):
        calls.append(v.numel())
        v.mul_(lam_t)

    for orth in ("MGS", "CGS", "DGKS"):
        ref = _ref(("len", N, orth), b, lam, restart=30, maxiter=100, orth=orth)
        x = np.zeros(N, complex)
        x, h = lsfc.gmres_(x, M, b, Pl=host if route == "host" else dev, Pl_on_device=route == "torch", restart=30,
                           maxiter=100, log=True, orth_meth=ORTH[orth])
        _check(f"{route} callback {orth}", x, h, ref)
    # one call per init and per step, none surplus (mvps leaves out the first init)
    assert len(calls) == sum(_REFS[("len", N, o_)]["mvps"] + 1 for o_ in ("MGS", "CGS", "DGKS")) and set(calls) == {N}


@pytest.mark.parametrize("orth", ["MGS", "CGS", "DGKS"])
def test_multi_device_plan(lsfc, orth):
    # four logical ranks on one GPU: the all-reduced blas_dot / blas_axpy_dot / blas_multidot / blas_nrm2 path, slabs of
    # 16 * 22 * 9 = 3168 entries (not a multiple of 1024)
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n, m, l = 16, 22, 36
    N = n * m * l
    M = MultiDeviceFastM3D(n, 1.0 / n, 3.0, np.zeros(N), devices=[0] * 4, m=m, l=l)
    try:
        x = gr.random_rhs(N, seed=9)
        assert np.array_equal((M * x).view(np.float64), x.view(np.float64))
        assert M.local_n == N // 4 and M.local_n % 1024 != 0
        lam, b = gr.disc_spectrum(N, 0.9, seed=10), gr.random_rhs(N, seed=11)

        def Pl(v):
            v *= lam

        ref = _ref(("multi", orth), b, lam, restart=65, maxiter=100, orth=orth)
        u = np.zeros(N, complex)
        u, h = lsfc.gmres_(u, M, b, Pl=Pl, restart=65, maxiter=100, log=True, orth_meth=ORTH[orth])
        _check(f"multi-device {orth}", u, h, ref)
    finally:
        M.close()


# -- exhausted Krylov space ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small-N1", "small-N2", "small-N3", "small-N5", "unit", "identity", "seven"])
@pytest.mark.parametrize("orth", ["MGS", "CGS", "DGKS"])
def test_exhausted_krylov_space(lsfc, plan, monkeypatch, kind, orth):
    N, m, lam, b, restart = gr.exhausted_problem(kind)
    gmap = None if m is None else gr.group_map(N, m)
    counts = None if m is None else gr.group_counts(gmap, m)
    lam_f, b_f = (lam, b) if m is None else (lam[gmap], b[gmap])
    ref = _ref(("exhausted", kind, orth), b, lam, counts=counts, restart=restart, orth=orth)
    M = plan(N)
    P = _diag_precond(lsfc, lam_f)
    try:
        x, h = _solve(lsfc, M, P, b_f, monkeypatch, orth, restart=restart)
    finally:
        P.close()
    label = f"{kind} {orth}"
    dim = np.unique(lam).size                                            # the Krylov dimension
    assert h.isconverged and 1 <= h.iters <= dim, f"{label}: converged={h.isconverged} after {h.iters} iterations " \
                                                  f"(history ends {np.asarray(h['resnorm'])[-3:]})"
    assert np.all(np.isfinite(x)), f"{label}: non-finite x"
    # diag(lam) x = diag(lam) b
    assert np.max(np.abs(lam_f * (x - b_f))) / np.max(np.abs(lam_f * b_f)) < 1e-12, label
    _check(label, x, h, ref, gmap)
