"""GPU tests of the lock-step BiCGStab(l) (lsfc_bicgstabl_batch, bicgstabl_batch_): every member of a batch against
bicgstabl_ on that member alone -- bit for bit on the identity operator of tests/test_gpu_bicgstabl.py with diag(lambda) as
preconditioner, where the batched applies are bitwise member-independent -- and against the long-double restatement where
tests/test_bicgstabl_batch_cases_cpu.py has checked the input condition.  "Bitwise" is np.array_equal on x, on the history
and on (iters, mvps, converged)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import bicgstabl_ref as br
import bicgstabl_batch_cases as bc
import cases
from conftest import rel_err
import krylov_common as kc
from krylov_common import _bitwise, _diag_precond, plan  # noqa: F401  (plan: the cached identity plans)

pytestmark = pytest.mark.gpu

_check = functools.partial(kc._check, history_excess=br.history_excess)


def _batch(lsfc, M, P, members, **over):
    """the members as one batch: rows b, x0 and r_shadow stacked, the shared options of member 0"""
    N, kw = M.N, dict(members[0])
    kw.update(over)
    shadow = bc.stack(members, "r_shadow", N) if members[0].get("r_shadow") is not None else None
    X = bc.stack(members, "x0", N)
    return lsfc.bicgstabl_batch_(X, M, bc.stack(members, "b", N), l=kw["l"], Pl=P, max_mv_products=kw.get("max_mv_products"),
                                 abstol=kw.get("abstol", 0.0), log=True, r_shadow=shadow,
                                 initially_zero=bool(kw.get("initially_zero", False)))


def _single(lsfc, M, P, kw):
    x = np.zeros(M.N, complex) if kw.get("x0") is None else np.array(kw["x0"], dtype=complex)
    return lsfc.bicgstabl_(x, M, np.array(kw["b"], dtype=complex), l=kw["l"], Pl=P, max_mv_products=kw.get("max_mv_products"),
                           abstol=kw.get("abstol", 0.0), log=True,
                           r_shadow=None if kw.get("r_shadow") is None else np.array(kw["r_shadow"], dtype=complex),
                           initially_zero=bool(kw.get("initially_zero", False)))


def _batch_is_the_single_solves(lsfc, M, P, members, tag):
    X, hs = _batch(lsfc, M, P, members)
    assert len(hs) == len(members)
    for j, kw in enumerate(members):
        x1, h1 = _single(lsfc, M, P, kw)
        _bitwise(tag, X, hs, j, x1, h1)
    return X, hs


# -- 1: member by member, at 1, 1, 2 and 65 reduction blocks -------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 65, 1025, 65538])
def test_member_by_member(lsfc, plan, N):
    M = plan(N)
    P = _diag_precond(lsfc, br.length_problem(N)[0])
    try:
        for l in (1, 2):
            X, hs = _batch_is_the_single_solves(lsfc, M, P, bc.length_members(N, l), f"N{N}-l{l}")
            assert all(h.iters > 0 for h in hs)
    finally:
        P.close()


# -- 2: the 1024-block cap of the reductions ------------------------------------------------------------------------------
def test_block_cap(lsfc, plan):
    N, m = (1 << 20) + 3, br.GROUPS
    gmap = br.group_map(N, m)
    lam, b = br.grouped_problem()
    members = [dict(b=b[gmap], pl=lam, l=2, max_mv_products=br.MAX_MV),
               dict(b=br.random_rhs(m, seed=5)[gmap], pl=lam, l=2, max_mv_products=br.MAX_MV)]
    M = plan(N)
    P = _diag_precond(lsfc, lam[gmap])
    try:
        X, hs = _batch_is_the_single_solves(lsfc, M, P, members, "block-cap")
    finally:
        P.close()
    first = np.zeros(m, dtype=np.int64)
    first[gmap[::-1]] = np.arange(N - 1, -1, -1)
    for j in range(2):
        # every group bitwise constant: an element that a tail skipped or updated twice breaks it
        x = X[j]
        bad = np.flatnonzero(np.any(x.view(np.float64).reshape(-1, 2) != x[first][gmap].view(np.float64).reshape(-1, 2), axis=1))
        assert bad.size == 0, f"member {j}: x is not constant on its groups: first index {bad[0] if bad.size else -1}"
        assert hs[j].isconverged and hs[j].iters > 3


# -- 3: members leave at different cycles: compaction of the active list, per-member tolerances -----------------------------
@pytest.mark.parametrize("l", [1, 2])
def test_members_leave_at_different_cycles(lsfc, plan, l):
    members = bc.leave_members(l)
    M = plan(bc.LEAVE_N)
    P = _diag_precond(lsfc, br.option_problem()[0])
    try:
        X, hs = _batch_is_the_single_solves(lsfc, M, P, members, f"leave-l{l}")
    finally:
        P.close()
    assert tuple(h.iters for h in hs) == bc.LEAVE_CYCLES[l]
    assert all(h.status[0] == lsfc._lib.LSFC_BICG_CONVERGED and h.isconverged and h.message == "" for h in hs)
    assert [h.status[1] for h in hs] == [h.iters for h in hs]
    for j, kw in enumerate(members[:5]):
        _check(f"leave-l{l}-member{j}", X[j], hs[j], br.bicgstabl_ref(**kw))
    assert (hs[5].iters, hs[5].mvps) == (0, 1) and not np.any(X[5]) and hs[5]["resnorm"].size == 0


# -- 4: more members than one operator group, and a batch of one --------------------------------------------------------
def test_groups(lsfc, plan):
    N = 1025
    M = plan(N)
    P = _diag_precond(lsfc, br.length_problem(N)[0])
    try:
        _batch_is_the_single_solves(lsfc, M, P, bc.length_members(N, 2, count=9), "nine")
        _batch_is_the_single_solves(lsfc, M, P, bc.length_members(N, 2, count=1), "one")
    finally:
        P.close()


# -- 5: every instance of the templated kernels ----------------------------------------------------------------------------
@pytest.mark.parametrize("l", range(1, 9))
def test_every_l(lsfc, plan, l):
    lam, b = br.large_l_problem()
    members = [dict(b=b, pl=lam, l=l, max_mv_products=br.MAX_MV), dict(b=br.random_rhs(1025, seed=1027), pl=lam, l=l, max_mv_products=br.MAX_MV)]
    P = _diag_precond(lsfc, lam)
    try:
        X, hs = _batch_is_the_single_solves(lsfc, plan(1025), P, members, f"l{l}")
    finally:
        P.close()
    assert all(h.isconverged and h.iters > 1 for h in hs)


# -- 6: a breakdown beside a healthy member ------------------------------------------------------------------------------------
def test_breakdown_beside_a_healthy_member(lsfc, plan):
    L = lsfc._lib
    members = bc.breakdown_members()
    M = plan(2)
    P = _diag_precond(lsfc, members[0]["pl"])
    try:
        X, hs = _batch(lsfc, M, P, members)
        msg = L.load().lsfc_last_error().decode()
        # the C return code
        Xc, Bc, Sc = bc.stack(members, "x0", 2), bc.stack(members, "b", 2), bc.stack(members, "r_shadow", 2)
        res, status = (L.GmresResult * 2)(), np.zeros(4, dtype=np.int64)
        opts = L.BicgstablOpts(l=1, max_mv_products=10, reltol=-1.0, r_shadow=Sc.ctypes.data_as(C.c_void_p))
        opts.precond, opts.precond_user, opts.precond_on_device = C.cast(L.load().lsfc_precond_callback, L.PRECOND_FN), P._pc, 1
        rc = L.load().lsfc_bicgstabl_batch(M._plan, Xc.ctypes.data_as(C.c_void_p), Bc.ctypes.data_as(C.c_void_p), 2, C.byref(opts), None, 0,
                                           res, status.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST)
    finally:
        P.close()
    assert rc == 0                                                       # LSFC_OK
    assert list(status) == [L.LSFC_BICG_SIGMA, 1, L.LSFC_BICG_CONVERGED, 2] and np.array_equal(Xc, X)
    # member 0: x0 untouched, the residual of x0 in the history
    assert np.array_equal(X[0], members[0]["x0"]) and np.array_equal(hs[0]["resnorm"], [0.75])
    assert hs[0].status == (L.LSFC_BICG_SIGMA, 1) and not hs[0].isconverged and (hs[0].iters, hs[0].mvps) == (1, 3)
    assert "breakdown in cycle 1" in hs[0].message and "sigma" in hs[0].message
    # member 1 is not touched by it
    ref = br.bicgstabl_ref(**members[1])
    assert ref["converged"] and (ref["iters"], ref["mvps"]) == (2, 5)
    assert hs[1].isconverged and (hs[1].iters, hs[1].mvps) == (2, 5) and hs[1].status[0] == L.LSFC_BICG_CONVERGED
    assert np.max(np.abs(X[1] - 1.0)) <= 1e-12
    assert "right-hand side 0" in msg and "sigma" in msg and "cycle 1" in msg


# -- 7: the cap ---------------------------------------------------------------------------------------------------------------
def test_cap(lsfc, plan):
    lam, b = br.option_problem()[:2]
    members = [dict(b=b, pl=lam, l=2, max_mv_products=14), dict(b=br.random_rhs(1025, seed=41), pl=lam, l=2, max_mv_products=14)]
    P = _diag_precond(lsfc, lam)
    try:
        X, hs = _batch_is_the_single_solves(lsfc, plan(1025), P, members, "cap")
    finally:
        P.close()
    for h in hs:
        assert not h.isconverged and h.status[0] == lsfc._lib.LSFC_BICG_MAX_MV and 14 <= h.mvps <= 18 and "max_mv_products" in h.message


# -- 8: options -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["shadow", "initially-zero"])
def test_options(lsfc, plan, option):
    lam, b, x0, shadow = br.option_problem()
    b2 = br.random_rhs(1025, seed=41)
    if option == "shadow":
        members = [dict(b=b, pl=lam, l=2, r_shadow=shadow), dict(b=b2, pl=lam, l=2, r_shadow=br.random_rhs(1025, seed=25))]
    else:
        members = [dict(b=b, pl=lam, l=2, x0=x0, initially_zero=True), dict(b=b2, pl=lam, l=2, x0=-x0, initially_zero=True)]
    P = _diag_precond(lsfc, lam)
    try:
        X, hs = _batch_is_the_single_solves(lsfc, plan(1025), P, members, option)
    finally:
        P.close()
    assert all(h.isconverged for h in hs)
    if option == "initially-zero":
        assert all(h.mvps == 4 * h.iters for h in hs)          # no product for the initial residual


# -- 9: routes ------------------------------------------------------------------------------------------------------------------
def test_routes(lsfc, plan):
    import torch
    N = 1025
    M = plan(N)
    lam = br.length_problem(N)[0]
    members = bc.length_members(N, 2)
    Bn = bc.stack(members, "b", N)
    P = _diag_precond(lsfc, lam)
    try:
        X, hs = _batch(lsfc, M, P, members)
        Xt = torch.zeros((3, N), dtype=torch.complex128, device="cuda")
        Xt2, ht = lsfc.bicgstabl_batch_(Xt, M, torch.from_numpy(Bn).cuda(), l=2, Pl=P, max_mv_products=br.length_cap(N), log=True)
        assert Xt2 is Xt
        for j in range(3):
            _bitwise("torch", Xt.cpu().numpy(), ht, j, X[j], hs[j])
    finally:
        P.close()
    calls = []

    def host(v):
        calls.append(v.size)
        v *= lam

    Xh, hh = lsfc.bicgstabl_batch_(np.zeros((3, N), complex), M, Bn, l=2, Pl=host, max_mv_products=br.length_cap(N), log=True)
    assert len(calls) == sum(h.mvps for h in hh) and set(calls) == {N}
    for j in range(3):
        _check(f"host route, member {j}", Xh[j], hh[j], br.bicgstabl_ref(**members[j]))

    def boom(v):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError):
        lsfc.bicgstabl_batch_(np.zeros((3, N), complex), M, Bn, Pl=boom)


# -- 10: the real operator ------------------------------------------------------------------------------------------------------
def test_real_operator(lsfc):
    c = cases.case_3d("gv16k10")
    Mo, n = c["M"], c["n"]
    M = lsfc.FastM3D(Mo.GFFT, Mo.nu, Mo.ne, Mo.me, Mo.le, n, n, n, Mo.omega)
    G2 = o.reduce_symbol(Mo.GFFT, (n, n, n))
    A = lambda v: o.apply_reduced(G2, Mo.nu, Mo.omega, v, (n, n, n))       # noqa: E731
    incs = [cases.plane_wave(c["k"], c["X"]), cases.plane_wave(c["k"], c["Y"])]
    rhs = np.array([-(M * u - u) for u in incs])
    U, hs = lsfc.bicgstabl_batch_(np.zeros((2, M.N), complex), M, rhs, l=2, reltol=1e-10, log=True)
    for j in range(2):
        ref = br.bicgstabl_ref(rhs[j], a=A, l=2, reltol=1e-10, dtype=np.complex128)
        res_ref = float(np.linalg.norm(A(ref["x"]) - rhs[j]) / np.linalg.norm(rhs[j]))
        res = float(np.linalg.norm(A(U[j]) - rhs[j]) / np.linalg.norm(rhs[j]))
        print(f"16^3 direction {j}: device {hs[j].iters} cycles, true residual {res:.3e}; fp64 restatement {ref['iters']} cycles, {res_ref:.3e}")
        assert ref["converged"] and hs[j].isconverged
        assert res <= 10 * res_ref
        assert abs(hs[j].iters - ref["iters"]) <= 1
    M.close()


# -- 11: the real operator with the device preconditioner --------------------------------------------------------------------
def test_real_operator_with_the_device_preconditioner(lsfc):
    from test_gpu_sparsify import case
    dims = (24, 24, 24)
    M, rows, nu, k, Mo = case("gv3", dims)
    N = int(np.prod(dims))
    x = -0.5 + np.arange(dims[0]) / dims[0]
    incs = [np.exp(1j * k * g) for g in o.grid3d(x, x, x)]
    rhs = np.array([-(M * u - u) for u in incs])
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    try:
        U, hs = lsfc.bicgstabl_batch_(np.zeros((3, N), complex), M, rhs, l=2, Pl=P, reltol=1e-10, log=True)
        info = P.batch_info()
        singles = [lsfc.bicgstabl_(np.zeros(N, complex), M, rhs[j], l=2, Pl=P, reltol=1e-10, log=True) for j in range(3)]
    finally:
        P.close()
    # the members met at the preconditioner
    assert info["sweeps"] > 0 and info["largest_group"] == 3, info
    # the yardstick of test_gpu_bicgstabl.test_real_operator_with_the_device_preconditioner: the fp64 restatement against the
    # oracle's GMRES, both with the same pair applied on the host (first direction)
    Msp, As = lsfc.sparsifying_pair(M)
    Po = o.SparsifyingPreconditioner(Msp, As)
    A = lambda v: o.mul(Mo, v)                                             # noqa: E731
    ref = br.bicgstabl_ref(rhs[0], a=A, pl=Po.solve, l=2, reltol=1e-10, dtype=np.complex128)
    uo, _ = o.gmres(np.zeros(N, complex), A, rhs[0], Pl=Po.solve, reltol=1e-10)
    yard = rel_err(ref["x"], uo)
    assert ref["converged"]
    for j in range(3):
        u1, h1 = singles[j]
        diff = rel_err(U[j], u1)
        print(f"gv3 24^3 direction {j}: batch {hs[j].mvps} mvps ({hs[j].iters} cycles), single {h1.mvps}; |x - x_single| {diff:.3e}, yardstick {yard:.3e}")
        assert hs[j].isconverged and h1.isconverged
        assert diff <= 10 * yard
    M.close()


# -- 12: errors -----------------------------------------------------------------------------------------------------------------
def test_errors(lsfc, plan):
    L = lsfc._lib
    N = 1025
    M = plan(N)
    X = np.zeros((65, N), complex)
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_batch_(X, M, np.ones((65, N), complex))
    assert ei.value.code == L.LSFC_EINVAL and "1..64" in str(ei.value) and not np.any(X)
    X = np.zeros((2, N), complex)
    with pytest.raises(ValueError):
        lsfc.bicgstabl_batch_(X, M, np.ones((3, N), complex))
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_batch_(X, M, np.ones((2, N), complex), l=9)
    assert ei.value.code == L.LSFC_EINVAL and "1..8" in str(ei.value)
    assert not np.any(X)
    # a multi-device plan (two logical ranks on one GPU) and a simulated rank of a slab plan
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n = 16
    Mm = MultiDeviceFastM3D(n, 1.0 / n, 3.0, np.zeros(n ** 3), devices=[0, 0])
    try:
        Xm = np.zeros((2, n ** 3), complex)
        with pytest.raises(lsfc.LsfcError) as ei:
            lsfc.bicgstabl_batch_(Xm, Mm, np.array([br.random_rhs(n ** 3), br.random_rhs(n ** 3)]))
        assert ei.value.code == L.LSFC_EINVAL and "single-device" in str(ei.value) and not np.any(Xm)
    finally:
        Mm.close()
    sim = C.c_void_p()
    nu = np.zeros(n * n * (n // 2))
    L.check(L.load().lsfc_dist_sim_plan_create_gv3d(C.byref(sim), n, n, n, 1.0, 3.0, nu.ctypes.data_as(C.c_void_p), 0, 0, 0, 2))
    try:
        xs, bs = np.zeros((2, nu.size), complex), np.array([br.random_rhs(nu.size), br.random_rhs(nu.size)])
        res = (L.GmresResult * 2)()
        opts = L.BicgstablOpts(l=2, reltol=-1.0)
        rc = L.load().lsfc_bicgstabl_batch(sim, xs.ctypes.data_as(C.c_void_p), bs.ctypes.data_as(C.c_void_p), 2, C.byref(opts), None, 0,
                                           res, None, L.LSFC_MEM_HOST)
        assert rc == L.LSFC_EINVAL and b"single-device" in L.load().lsfc_last_error() and not np.any(xs)
    finally:
        L.load().lsfc_plan_destroy(sim)
