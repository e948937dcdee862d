"""GPU tests of the device BiCGStab(l) (csrc/bicgstab.hip) against the long-double restatement of tests/bicgstabl_ref.py.

The operator of the kernel tests is that of tests/test_gpu_gmres_kernels.py: a plan with a ones symbol and nu == 0, so that
M * x == x bitwise, and the left preconditioner diag(lambda) -- BiCGStab(l) then iterates on exactly diag(lambda) and only
the reductions see the order of summation.  Criteria of that suite: history within gmres_ref.history_excess < 1 at rtol
1e-10 (ten times the input condition that tests/test_bicgstabl_ref_cpu.py checks for every problem used here), x within
1e-10, iters / mvps / converged equal (one cycle apart only where the reference stops within 1e-8 of the tolerance).
The real-operator tests run the 3D 16^3 golden problem and the preconditioned systems of tests/test_gpu_sparsify.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import bicgstabl_ref as br
import cases
from conftest import rel_err
import krylov_common as kc
from krylov_common import _diag_precond, plan  # noqa: F401  (plan: the cached identity plans)

pytestmark = pytest.mark.gpu


_CASES = br.gpu_cases()
_REFS = {}


def _ref(label):
    """the long-double reference of a problem of bicgstabl_ref.gpu_cases(), computed once"""
    if label not in _REFS:
        _REFS[label] = br.bicgstabl_ref(**_CASES[label])
    return _REFS[label]


_check = functools.partial(kc._check, history_excess=br.history_excess)


def _run(lsfc, M, label, P, gmap=None, **over):
    """the problem `label` on the device: b, x0, r_shadow expanded to the full vector, the reference's options"""
    kw = dict(_CASES[label])
    kw.update(over)
    ex = (lambda v: np.asarray(v)) if gmap is None else (lambda v: np.asarray(v)[gmap])
    x = np.zeros(M.N, complex) if kw.get("x0") is None else np.array(ex(kw["x0"]), dtype=complex)
    return lsfc.bicgstabl_(x, M, np.array(ex(kw["b"]), dtype=complex), l=kw["l"], Pl=P,
                           max_mv_products=kw.get("max_mv_products"), log=True,
                           r_shadow=None if kw.get("r_shadow") is None else np.array(ex(kw["r_shadow"]), dtype=complex),
                           initially_zero=bool(kw.get("initially_zero", False)))


# -- vector lengths: reduction tails and block boundaries ---------------------------------------------------------------
@pytest.mark.parametrize("N", br.LENGTHS)
def test_vector_lengths(lsfc, plan, N):
    M = plan(N)
    P = _diag_precond(lsfc, br.length_problem(N)[0])
    try:
        for l in (1, 2):
            label = f"len-N{N}-l{l}"
            x, h = _run(lsfc, M, label, P)
            _check(label, x, h, _ref(label))
    finally:
        P.close()


# -- larger l: every instance of the templated kernels -------------------------------------------------------------------
@pytest.mark.parametrize("l", br.LARGE_L)
def test_larger_l(lsfc, plan, l):
    M = plan(1025)
    P = _diag_precond(lsfc, br.large_l_problem()[0])
    try:
        x, h = _run(lsfc, M, f"large-l{l}", P)
        _check(f"large-l{l}", x, h, _ref(f"large-l{l}"))
    finally:
        P.close()


def _solves_and_repeats(lsfc, M, lam, b, l, label):
    """criteria that need no history bound, for problems outside the input condition: the solve converges, everything is
    finite, a second solve is bitwise the first, and the true residual of the preconditioned system is within 2 tol (the
    recursive residual is <= tol at convergence; its gap to the true one is O(cycles eps |lam| |x|) ~ 1e-13 beta0 << tol)"""
    N = b.size
    P = _diag_precond(lsfc, lam)
    try:
        x, h = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=l, Pl=P, max_mv_products=br.MAX_MV, log=True)
        x1, h1 = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=l, Pl=P, max_mv_products=br.MAX_MV, log=True)
    finally:
        P.close()
    r = np.asarray(h["resnorm"])
    assert h.isconverged, f"{label}: {h.iters} cycles, {h.mvps} mvps, {r[-3:]} ({h.message})"
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(r)), label
    assert np.array_equal(x, x1) and np.array_equal(r, np.asarray(h1["resnorm"])), f"{label}: not repeatable"
    tol = br.DEFAULT_RELTOL * np.linalg.norm(lam * b)
    res = np.linalg.norm(lam * (b - x))
    print(f"{label}: {h.iters} cycles, {h.mvps} mvps, true residual {res / tol:.3f} tol")
    assert r[-1] <= tol * (1 + 1e-12) and res <= 2 * tol, f"{label}: true residual {res:.3e}, tol {tol:.3e}"
    return x, h


@pytest.mark.parametrize("l", br.WIDE_L)
def test_wide_l_solves(lsfc, plan, l):
    # l = 5 ... 8 break the 1e-11 input condition on this problem (the largest l that keeps it is 4, test_larger_l), so there
    # is no history comparison: these instances of the templated kernels are held to what needs no loosened bound
    lam, b = br.large_l_problem()
    _solves_and_repeats(lsfc, plan(1025), lam, b, l, f"wide-l{l}")


@pytest.mark.parametrize("N", [63, 64, 65])
def test_short_lengths_to_convergence(lsfc, plan, N):
    # test_vector_lengths stops these lengths at 40 products (beyond that the input condition breaks: the space has fewer
    # dimensions than convergence at rho = 0.9 needs products); here they run to convergence, without a history comparison
    lam, b = br.length_problem(N)
    for l in (1, 2):
        _solves_and_repeats(lsfc, plan(N), lam, b, l, f"short-N{N}-l{l}")


# -- large N: the 1024-block cap of the reductions -----------------------------------------------------------------------
@pytest.mark.parametrize("N", br.GROUPED)
def test_large_grouped(lsfc, plan, N):
    m = br.GROUPS
    gmap = br.group_map(N, m)
    label = f"grouped-N{N}"
    M = plan(N)
    P = _diag_precond(lsfc, br.grouped_problem()[0][gmap])
    try:
        x, h = _run(lsfc, M, label, P, gmap=gmap)
    finally:
        P.close()
    # every group bitwise constant: an element that a tail skipped or updated twice breaks it
    first = np.zeros(m, dtype=np.int64)
    first[gmap[::-1]] = np.arange(N - 1, -1, -1)
    bad = np.flatnonzero(np.any(x.view(np.float64).reshape(-1, 2) != x[first][gmap].view(np.float64).reshape(-1, 2), axis=1))
    assert bad.size == 0, f"{label}: x is not constant on its groups: first index {bad[0]}, {bad.size} entries differ"
    assert h.isconverged
    _check(label, x, h, _ref(label), gmap)


# -- exhausted Krylov space ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3])
def test_exhausted_space(lsfc, plan, N):
    lam, b = br.disc_spectrum(N, 0.9, seed=N), br.random_rhs(N, seed=N + 1)
    M = plan(N)
    P = _diag_precond(lsfc, lam)
    try:
        x, h = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=2, Pl=P, max_mv_products=20, log=True)
    finally:
        P.close()
    assert h.isconverged, (h.iters, h.mvps, h["resnorm"], h.message)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(h["resnorm"]))
    assert np.linalg.norm(lam * (b - x)) <= 1e-8 * np.linalg.norm(lam * b)


# -- bitwise equalities and the routes to the preconditioner --------------------------------------------------------------
def test_repeated_solves_are_bitwise_equal(lsfc, plan):
    N = 4095
    M = plan(N)
    lam, b = br.length_problem(N)
    P = _diag_precond(lsfc, lam)
    try:
        for l in (1, 2, 4):
            x0, h0 = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=l, Pl=P, max_mv_products=100, log=True)
            x1, h1 = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=l, Pl=P, max_mv_products=100, log=True)
            assert h0.iters > 3 and np.array_equal(h0["resnorm"], h1["resnorm"]) and np.array_equal(x0, x1), l
    finally:
        P.close()


@pytest.mark.parametrize("label", ["shadow", "x0", "x0-initially-zero", "cap"])
def test_options(lsfc, plan, label):
    N = 1025
    M = plan(N)
    P = _diag_precond(lsfc, br.option_problem()[0])
    try:
        x, h = _run(lsfc, M, label, P)
    finally:
        P.close()
    ref = _ref(label)
    _check(label, x, h, ref)
    if label == "cap":
        cap, l = _CASES[label]["max_mv_products"], _CASES[label]["l"]
        assert not h.isconverged and cap <= h.mvps <= cap + 2 * l and "max_mv_products" in h.message
    else:
        assert h.isconverged


@pytest.mark.parametrize("route", ["host", "torch", "torch-vectors"])
def test_callback_routes(lsfc, plan, route):
    import torch
    N = 1025
    M = plan(N)
    label = "len-N1025-l2"
    lam, b = br.length_problem(N)
    lam_t = torch.from_numpy(lam).cuda()
    calls = []

    def host(v):
        calls.append(v.size)
        v *= lam

    def dev(v):
        calls.append(v.numel())
        v.mul_(lam_t)

    P = _diag_precond(lsfc, lam)
    try:
        xp, hp = _run(lsfc, M, label, P)
        if route == "torch-vectors":                # x and b on the device, the preconditioner object: same bits
            xt = torch.zeros(N, dtype=torch.complex128, device="cuda")
            xt, h = lsfc.bicgstabl_(xt, M, torch.from_numpy(b).cuda(), l=2, Pl=P, max_mv_products=br.length_cap(N), log=True)
            x = xt.cpu().numpy()
        else:
            x, h = lsfc.bicgstabl_(np.zeros(N, complex), M, b, l=2, Pl=host if route == "host" else dev,
                                   Pl_on_device=route == "torch", max_mv_products=br.length_cap(N), log=True)
    finally:
        P.close()
    ref = _ref(label)
    _check(f"{route} route", x, h, ref)
    if route == "torch-vectors":                    # the same object on the same kernels: bitwise the host-vector solve
        assert np.array_equal(h["resnorm"], hp["resnorm"]) and np.array_equal(x, xp), route
    else:                    # one call for the initial residual, one per operator application
        assert len(calls) == ref["mvps"] and set(calls) == {N}

    def boom(v):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError):
        lsfc.bicgstabl_(np.zeros(N, complex), M, b, Pl=boom)


# -- the real operator ---------------------------------------------------------------------------------------------------
def test_real_operator_without_preconditioner(lsfc):
    c = cases.case_3d("gv16k10")
    Mo, n = c["M"], c["n"]
    M = lsfc.FastM3D(Mo.GFFT, Mo.nu, Mo.ne, Mo.me, Mo.le, n, n, n, Mo.omega)
    u_inc = cases.plane_wave(c["k"], c["X"])
    rhs = -(M * u_inc - u_inc)
    G2 = o.reduce_symbol(Mo.GFFT, (n, n, n))
    A = lambda v: o.apply_reduced(G2, Mo.nu, Mo.omega, v, (n, n, n))       # noqa: E731
    ref = br.bicgstabl_ref(rhs, a=A, l=2, reltol=1e-10, dtype=np.complex128)
    res_ref = float(np.linalg.norm(A(ref["x"]) - rhs) / np.linalg.norm(rhs))
    u, h = lsfc.bicgstabl_(np.zeros(M.N, complex), M, rhs, l=2, reltol=1e-10, log=True)
    res = float(np.linalg.norm(A(u) - rhs) / np.linalg.norm(rhs))
    print(f"16^3: device {h.iters} cycles, true residual {res:.3e}; fp64 restatement {ref['iters']} cycles, {res_ref:.3e}")
    assert ref["converged"] and h.isconverged
    assert res <= 10 * res_ref
    assert abs(h.iters - ref["iters"]) <= 1
    M.close()


@pytest.mark.parametrize("kind,dims", [("trap", (101, 101, 1)), ("gv3", (24, 24, 24))])
def test_real_operator_with_the_device_preconditioner(lsfc, kind, dims):
    from test_gpu_sparsify import case
    M, rows, nu, k, Mo = case(kind, dims)
    N = int(np.prod(dims))
    if kind == "trap":
        X = o.grid2d(*(2 * [-0.5 + np.arange(dims[0]) / (dims[0] - 1)]))[0]
        u_inc = np.exp(1j * k * X)
        rhs = -k ** 2 * lsfc.FFTconvolution(M, nu * u_inc)
    else:
        x = -0.5 + np.arange(dims[0]) / dims[0]
        u_inc = np.exp(1j * k * o.grid3d(x, x, x)[0])
        rhs = -(M * u_inc - u_inc)
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    try:
        u, h = lsfc.bicgstabl_(np.zeros(N, complex), M, rhs, l=2, Pl=P, reltol=1e-10, log=True)
        ug, hg = lsfc.gmres_(np.zeros(N, complex), M, rhs, Pl=P, reltol=1e-10, log=True)
    finally:
        P.close()
    u0, h0 = lsfc.bicgstabl_(np.zeros(N, complex), M, rhs, l=2, reltol=1e-10, max_mv_products=4000, log=True)
    # the yardstick: the fp64 restatement against the oracle's GMRES, both with the same pair applied on the host
    Msp, As = lsfc.sparsifying_pair(M)
    Po = o.SparsifyingPreconditioner(Msp, As)
    A = lambda v: o.mul(Mo, v)                                             # noqa: E731
    ref = br.bicgstabl_ref(rhs, a=A, pl=Po.solve, l=2, reltol=1e-10, dtype=np.complex128)
    uo, _ = o.gmres(np.zeros(N, complex), A, rhs, Pl=Po.solve, reltol=1e-10)
    yard = rel_err(ref["x"], uo)
    diff = rel_err(u, ug)
    print(f"{kind} {dims}: bicgstabl {h.mvps} mvps ({h.iters} cycles) preconditioned, {h0.mvps} without; gmres {hg.mvps} mvps; "
          f"|x - x_gmres| {diff:.3e}, restatement against the oracle's GMRES {yard:.3e}")
    assert h.isconverged and hg.isconverged and ref["converged"]
    assert diff <= 10 * yard
    assert h.mvps < h0.mvps
    M.close()


# -- breakdown -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memspace", ["host", "device"])
def test_breakdown_keeps_the_last_finite_iterate(lsfc, plan, memspace):
    # a shadow residual orthogonal to the residual: rho == 0, then sigma == <r~, Pl A us[0]> == 0 in the first BiCG step of
    # cycle 1 -- k_bicg_rx sets the status word, every later update of the cycle is skipped, x stays x0 bit for bit
    import torch
    L = lsfc._lib
    M = plan(2)
    lam = np.array([1.0, 2.0], complex)
    b, shadow, x0 = np.array([1.0, 0.0], complex), np.array([0.0, 1.0], complex), np.array([0.25, 0.0], complex)
    ref = br.bicgstabl_ref(b, pl=lam, l=1, r_shadow=shadow, x0=x0, max_mv_products=10)
    assert ref["breakdown"] == "sigma" and not ref["converged"] and ref["iters"] == 1
    P = _diag_precond(lsfc, lam)
    try:
        if memspace == "device":
            xt = torch.from_numpy(x0.copy()).cuda()
            xt, h = lsfc.bicgstabl_(xt, M, torch.from_numpy(b).cuda(), l=1, Pl=P, r_shadow=torch.from_numpy(shadow).cuda(),
                                    max_mv_products=10, log=True)
            x = xt.cpu().numpy()
        else:
            x, h = lsfc.bicgstabl_(x0.copy(), M, b, l=1, Pl=P, r_shadow=shadow, max_mv_products=10, log=True)
        # the C return code and message
        xc, res = x0.copy(), L.GmresResult()
        opts = L.BicgstablOpts(l=1, max_mv_products=10, reltol=-1.0, r_shadow=shadow.ctypes.data_as(C.c_void_p))
        opts.precond, opts.precond_user, opts.precond_on_device = C.cast(L.load().lsfc_precond_callback, L.PRECOND_FN), P._pc, 1
        rc = L.load().lsfc_bicgstabl(M._plan, xc.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0,
                                     C.byref(res), L.LSFC_MEM_HOST)
        msg = L.load().lsfc_last_error().decode()
    finally:
        P.close()
    assert not h.isconverged and (h.iters, h.mvps) == (ref["iters"], ref["mvps"]) == (1, 3)
    assert np.array_equal(x, x0) and np.array_equal(xc, x0), (x, xc)
    assert np.array_equal(h["resnorm"], [0.75])                                     # ||lam (b - x0)||, exact in double
    assert "breakdown in cycle 1" in h.message and "sigma" in h.message
    assert rc == L.LSFC_ENOTCONV and "breakdown in cycle 1" in msg and "sigma" in msg and res.converged == 0


# -- errors --------------------------------------------------------------------------------------------------------------
def test_errors(lsfc, plan):
    L = lsfc._lib
    M = plan(1025)
    b = br.random_rhs(1025, seed=2)
    for l in (0, 9):
        with pytest.raises(lsfc.LsfcError) as ei:
            lsfc.bicgstabl_(np.zeros(1025, complex), M, b, l=l)
        assert ei.value.code == L.LSFC_EINVAL and "1..8" in str(ei.value)
    x = np.zeros(1025, complex)
    res = L.GmresResult()
    opts = L.BicgstablOpts(l=2, reltol=-1.0)
    opts.reserved[2] = 1
    args = (M._plan, x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0, C.byref(res))
    assert L.load().lsfc_bicgstabl(*args, L.LSFC_MEM_HOST) == L.LSFC_EINVAL and b"reserved" in L.load().lsfc_last_error()
    opts.reserved[2] = 0
    assert L.load().lsfc_bicgstabl(*args, 7) == L.LSFC_EINVAL and b"memspace" in L.load().lsfc_last_error()
    assert np.all(x == 0)
    # a multi-device plan (two logical ranks on one GPU) and a simulated rank of a slab plan
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n = 16
    Mm = MultiDeviceFastM3D(n, 1.0 / n, 3.0, np.zeros(n ** 3), devices=[0, 0])
    try:
        with pytest.raises(lsfc.LsfcError) as ei:
            lsfc.bicgstabl_(np.zeros(n ** 3, complex), Mm, br.random_rhs(n ** 3))
        assert ei.value.code == L.LSFC_EINVAL and "single-device" in str(ei.value)
    finally:
        Mm.close()
    sim = C.c_void_p()
    nu = np.zeros(n * n * (n // 2))
    L.check(L.load().lsfc_dist_sim_plan_create_gv3d(C.byref(sim), n, n, n, 1.0, 3.0, nu.ctypes.data_as(C.c_void_p), 0, 0, 0, 2))
    try:
        xs, bs = np.zeros(nu.size, complex), br.random_rhs(nu.size)
        opts = L.BicgstablOpts(l=2, reltol=-1.0)
        rc = L.load().lsfc_bicgstabl(sim, xs.ctypes.data_as(C.c_void_p), bs.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0,
                                     C.byref(res), L.LSFC_MEM_HOST)
        assert rc == L.LSFC_EINVAL and b"single-device" in L.load().lsfc_last_error()
    finally:
        L.load().lsfc_plan_destroy(sim)
