"""GPU tests that pin lsfc_gmres_batch (gmres_batch_): every member of a batch against gmres_ on that row alone, bit for
bit, on the identity operator of tests/test_gpu_bicgstabl.py with diag(lambda) as the device preconditioner.  On that
pipeline (LSFC_FLAG_FORCE_ROCFFT) the batched apply is a loop over the members, so a member's bits cannot depend on its
neighbours, and the single solve (which posts one step ahead) and the batch (which does not) run the same kernels on the
same data.  "Bitwise" is np.array_equal on x viewed as float64, on the history and on (iters, mvps, converged).
The inputs of items 1-4 come from pinned_cases() so that two builds of the library can be run on the same inputs."""
import threading

import numpy as np
import pytest

import cases
import gmres_ref as gr
from krylov_common import _bitwise, _diag_precond, plan  # noqa: F401  (plan: the cached identity plans)

pytestmark = pytest.mark.gpu

ORTH = {"MGS": "ModifiedGramSchmidt", "CGS": "ClassicalGramSchmidt", "DGKS": "DGKS"}
LENGTHS = [5, 65, 1025, 65538]          # 1, 1, 2 and 65 reduction blocks
RHO = 0.6                               # spectrum of diag(lambda): the disc |z - 1| <= RHO, some 35 iterations to sqrt(eps)
MAXITER = 80


def _lam(N):
    return gr.disc_spectrum(N, RHO, seed=N)


def _rows(N, nrhs):
    return np.stack([gr.random_rhs(N, seed=N + 1 + j) for j in range(nrhs)])


def _leave_rows(N):
    """a generic row, the same vector small enough for abstol to stop it several iterations earlier, and b = 0"""
    b = gr.random_rhs(N, seed=N + 1)
    return np.stack([b, 1e-3 * b, np.zeros(N, complex)])


LEAVE_ABSTOL = 1e-6     # row 0: beta0 ~ 50, tol = max(sqrt(eps) beta0, abstol) = 1e-6, 2e-8 beta0; row 1: 2e-5 of its beta0


def pinned_cases():
    """[(tag, N, B, X0 or None, keyword arguments of gmres_ / gmres_batch_)] of items 1-4; lambda is _lam(N)"""
    out = []
    for N in LENGTHS:                                                                   # 1: member equals single solve
        for orth in ORTH:
            for restart in (3, 20):
                out.append((f"member-N{N}-{orth}-r{restart}", N, _rows(N, 3), None, dict(orth_meth=ORTH[orth], restart=restart, maxiter=MAXITER)))
    out.append(("two-groups", 1025, _rows(1025, 11), None, dict(restart=20, maxiter=MAXITER)))    # 2: groups of 8 and 3
    N = 1025                                                                            # 3: members leave at different rounds
    for zero in (False, True):
        out.append((f"leave-zero{int(zero)}", N, _leave_rows(N), None, dict(restart=5, maxiter=MAXITER, abstol=LEAVE_ABSTOL, initially_zero=zero)))
    X0 = np.zeros((3, N), complex)
    X0[0] = 0.5 * gr.random_rhs(N, seed=77)
    out.append(("leave-x0", N, _leave_rows(N), X0, dict(restart=5, maxiter=MAXITER, abstol=LEAVE_ABSTOL, initially_zero=False)))
    out.append(("cap", N, _rows(N, 3), None, dict(restart=3, maxiter=7)))               # 4: restart boundary and cap
    return out


_CASES = {c[0]: c for c in pinned_cases()}
_SINGLES = {}


def _single(lsfc, M, P, tag, j):
    """gmres_ on row j of a pinned case, computed once"""
    if (tag, j) not in _SINGLES:
        _, N, B, X0, kw = _CASES[tag]
        x = np.zeros(N, complex) if X0 is None else X0[j].copy()
        _SINGLES[(tag, j)] = lsfc.gmres_(x, M, B[j].copy(), Pl=P, log=True, **kw)
    return _SINGLES[(tag, j)]


def _batch(lsfc, M, P, tag):
    _, N, B, X0, kw = _CASES[tag]
    X = np.zeros_like(B) if X0 is None else X0.copy()
    return lsfc.gmres_batch_(X, M, B.copy(), Pl=P, log=True, **kw)


def _batch_is_the_single_solves(lsfc, M, P, tag):
    X, hs = _batch(lsfc, M, P, tag)
    assert len(hs) == X.shape[0]
    for j in range(X.shape[0]):
        x1, h1 = _single(lsfc, M, P, tag, j)
        _bitwise(tag, X, hs, j, x1, h1)
    return X, hs


# -- 1: member equals single solve, at 1, 1, 2 and 65 reduction blocks, every orthogonalisation, two restart lengths --------
@pytest.mark.parametrize("N", LENGTHS)
def test_member_equals_single_solve(lsfc, plan, N):
    M = plan(N)
    P = _diag_precond(lsfc, _lam(N))
    try:
        for orth in ORTH:
            for restart in (3, 20):
                X, hs = _batch_is_the_single_solves(lsfc, M, P, f"member-N{N}-{orth}-r{restart}")
                assert all(h.iters > 0 for h in hs)
    finally:
        P.close()


# -- 2: more members than one operator group --------------------------------------------------------------------------------
def test_two_groups(lsfc, plan):
    M = plan(1025)
    P = _diag_precond(lsfc, _lam(1025))
    try:
        X, hs = _batch_is_the_single_solves(lsfc, M, P, "two-groups")
        X2, hs2 = _batch(lsfc, M, P, "two-groups")
    finally:
        P.close()
    assert X.shape[0] == 11
    for j in range(11):
        _bitwise("two-groups, second run", X2, hs2, j, X[j], hs[j])


# -- 3: members leave at different rounds -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["leave-zero0", "leave-zero1", "leave-x0"])
def test_members_leave_at_different_rounds(lsfc, plan, tag):
    M = plan(1025)
    P = _diag_precond(lsfc, _lam(1025))
    try:
        X, hs = _batch_is_the_single_solves(lsfc, M, P, tag)
    finally:
        P.close()
    iters = [h.iters for h in hs]
    print(f"{tag}: iterations {iters}, mvps {[h.mvps for h in hs]}")
    assert len(set(iters)) == 3 and iters[2] == 0 and iters[1] < iters[0]
    assert all(h.isconverged for h in hs)
    assert np.array_equal(X[2], np.zeros(1025))                  # b = 0: converged before the loop, x untouched


# -- 4: restart boundary and cap -----------------------------------------------------------------------------------------------
def test_restart_boundary_and_cap(lsfc, plan):
    M = plan(1025)
    P = _diag_precond(lsfc, _lam(1025))
    try:
        X, hs = _batch_is_the_single_solves(lsfc, M, P, "cap")      # (raises unless rc == LSFC_OK)
    finally:
        P.close()
    for h in hs:
        assert h.iters == 7 and not h.isconverged


# -- 5: callback routes -------------------------------------------------------------------------------------------------------
def test_host_callable_runs_on_the_callers_thread(lsfc, plan):
    N = 1025
    M, lam, B = plan(N), _lam(N), _rows(N, 3)
    calls = []

    def host(v):
        calls.append(threading.get_ident())
        v *= lam

    kw = dict(restart=5, maxiter=MAXITER, log=True)
    singles = [lsfc.gmres_(np.zeros(N, complex), M, B[j].copy(), Pl=host, **kw) for j in range(3)]
    alone = len(calls)
    del calls[:]
    X, hs = lsfc.gmres_batch_(np.zeros_like(B), M, B.copy(), Pl=host, **kw)
    assert len(calls) == alone
    for j in range(3):
        x1, h1 = singles[j]
        assert hs[j].iters == h1.iters and float(np.linalg.norm(X[j] - x1) / np.linalg.norm(x1)) < 1e-10
    assert set(calls) == {threading.get_ident()}, "the callback ran on a thread that is not the caller's"


def test_members_meet_at_the_device_preconditioner(lsfc):
    from test_gpu_precond_batch import _blocktri, _plane_wave_rhs
    kind, dims = "gv3", (16, 16, 16)
    M, RHS = _plane_wave_rhs(lsfc, kind, dims)
    P = _blocktri(lsfc, kind, dims)[0]
    try:
        X, hs = lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, Pl=P, reltol=1e-6, log=True)
        info = P.batch_info()
    finally:
        P.close()
    assert all(h.isconverged for h in hs)
    assert info["largest_group"] == 3 and info["sweeps"] > 0, info


# -- 6: errors leave the plan usable ------------------------------------------------------------------------------------------
def test_errors_leave_the_plan_usable(lsfc, plan):
    L = lsfc._lib
    N, tag = 1025, "member-N1025-MGS-r20"
    M, lam, B = plan(N), _lam(N), _CASES[tag][2]
    kw = _CASES[tag][4]
    count, fail_at = [0], [None]

    def host(v):
        count[0] += 1
        if count[0] == fail_at[0]:
            raise RuntimeError("fifth call")
        v *= lam

    Xg, hg = lsfc.gmres_batch_(np.zeros_like(B), M, B.copy(), Pl=host, log=True, **kw)
    assert count[0] > 5
    count[0], fail_at[0] = 0, 5
    with pytest.raises(RuntimeError, match="fifth call"):
        lsfc.gmres_batch_(np.zeros_like(B), M, B.copy(), Pl=host, **kw)
    fail_at[0] = None
    # the same plan afterwards: the host callable as before the failure, and the device object of item 1
    Xa, ha = lsfc.gmres_batch_(np.zeros_like(B), M, B.copy(), Pl=host, log=True, **kw)
    for j in range(3):
        _bitwise("host callable after the failure", Xa, ha, j, Xg[j], hg[j])
    P = _diag_precond(lsfc, lam)
    try:
        _batch_is_the_single_solves(lsfc, M, P, tag)
    finally:
        P.close()
    for nrhs in (0, 65):
        with pytest.raises(lsfc.LsfcError) as ei:
            lsfc.gmres_batch_(np.zeros((nrhs, N), complex), M, np.ones((nrhs, N), complex))
        assert ei.value.code == L.LSFC_EINVAL and "1..64" in str(ei.value)


# -- 7: the real operator: two runs of the batch are bitwise equal -----------------------------------------------------------
def real_operator_batch(lsfc):
    """the three incident directions of tests/test_gpu_batch.py on gv16k10 (pruned pipeline, fused batch pass)"""
    c = cases.case_3d("gv16k10")
    k = c["k"]
    M = lsfc.buildFastConvolution3D(c["x"], c["x"], c["x"], c["X"], c["Y"], c["Z"], c["h"], k, c["nu"])
    U_inc = np.stack([np.exp(1j * k * c["X"]), np.exp(1j * k * (0.6 * c["Y"] + 0.8 * c["Z"])), 0.01 * np.exp(1j * k * c["Z"])])
    RHS = -(lsfc.apply_batch(M, U_inc, 0) - U_inc)
    return M, RHS, dict(restart=5, reltol=1e-9, abstol=2e-8)


def test_real_operator_is_repeatable(lsfc):
    M, RHS, kw = real_operator_batch(lsfc)
    try:
        X1, h1 = lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, log=True, **kw)
        X2, h2 = lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, log=True, **kw)
    finally:
        M.close()
    for j in range(3):
        _bitwise("gv16k10, second run", X2, h2, j, X1[j], h1[j])
    assert all(h.isconverged for h in h1)
