"""GPU tests of BiCGStab(l) on a single-process multi-device plan (bicgstabl_multi_, lsfc_bicgstabl_multi; csrc/bicgstab.hip, the
team form; bicgstabl_ itself keeps refusing such a plan, tests/test_gpu_bicgstabl.py): the vectors cut into
the z slabs of P ranks, every sum completed in two levels (rank sums, copied into a table on every rank, added in rank order).

All plans are MultiDeviceFastM3D(..., devices=[0] * P): P logical ranks on one GPU, the copy transport.  The kernel tests use
nu == 0, so that M * x == x bitwise, and the host preconditioner v *= lambda: BiCGStab(l) iterates on exactly diag(lambda) and
only the reductions see the slabs.  Criteria of tests/test_gpu_bicgstabl.py: history within history_excess < 1 at rtol 1e-10
(ten times the input condition that tests/test_bicgstabl_multi_cases_cpu.py checks for every problem used here), x within
1e-10, iters / mvps / converged equal (one cycle apart only where the reference stops within 1e-8 of the tolerance)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import bicgstabl_ref as br
import bicgstabl_multi_cases as mc
import cases
import krylov_common as kc

pytestmark = pytest.mark.gpu

_check = functools.partial(kc._check, history_excess=br.history_excess)
_CASES = mc.cases()
_REFS = {}
_PLANS = {}


def _ref(label):
    """the long-double reference of a problem of bicgstabl_multi_cases.cases(), computed once"""
    if label not in _REFS:
        _REFS[label] = br.bicgstabl_ref(**_CASES[label][0])
    return _REFS[label]


@pytest.fixture(scope="module")
def identity(lsfc):
    """identity(grid, P) -> a cached plan with nu == 0 whose apply is the identity, bitwise: on P ranks (a multi-device
    plan, P >= 1), or P = None: the single-device plan of the same shape"""
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D

    def get(grid, P):
        if (grid, P) not in _PLANS:
            n, m, l = grid
            N, h = n * m * l, 1.0 / n
            if P is None:
                x = -0.5 + h * np.arange(n)
                M = lsfc.buildFastConvolution3D(x, x[:m], x[:l], None, None, None, h, 3.0, np.zeros(N))
            else:
                M = MultiDeviceFastM3D(n, h, 3.0, np.zeros(N), devices=[0] * P, m=m, l=l)
            x = br.random_rhs(N, seed=N)
            assert np.array_equal((M * x).view(np.float64), x.view(np.float64)), f"M * x != x on {grid}, P = {P}"
            _PLANS[(grid, P)] = M
        return _PLANS[(grid, P)]
    yield get
    for M in _PLANS.values():
        M.close()
    _PLANS.clear()


def _scale_by(lam, calls=None):
    """the host preconditioner v *= lam on the whole vector"""
    def Pl(v):
        if calls is not None:
            calls.append(v.size)
        v *= lam
    return Pl


def _solver(lsfc, M):
    """bicgstabl_multi_ on a multi-device plan, bicgstabl_ on the single-device one it is compared with"""
    return lsfc.bicgstabl_multi_ if hasattr(M, "devices") else lsfc.bicgstabl_


def _run(lsfc, M, label, **over):
    """the problem `label` on the device: b, x0, r_shadow and lambda expanded to the full vector, the reference's options"""
    kw, gmap = _CASES[label]
    kw = dict(kw, **over)
    ex = lambda v: np.array(np.asarray(v)[gmap], dtype=complex)                     # noqa: E731
    x = np.zeros(M.N, complex) if kw.get("x0") is None else ex(kw["x0"])
    return _solver(lsfc, M)(x, M, ex(kw["b"]), l=kw["l"], Pl=_scale_by(ex(kw["pl"])), max_mv_products=kw.get("max_mv_products"),
                           log=True, r_shadow=None if kw.get("r_shadow") is None else ex(kw["r_shadow"]),
                           initially_zero=bool(kw.get("initially_zero", False)))


# -- 1: the identity operator, history against the long-double reference ------------------------------------------------------
@pytest.mark.parametrize("l", mc.LS)
@pytest.mark.parametrize("grid,P", mc.GRIDS)
def test_history_against_the_reference(lsfc, identity, grid, P, l):
    M = identity(grid, P)
    label = mc.grouped_label(M.N, l)
    x, h = _run(lsfc, M, label)
    assert h.isconverged, h.message
    _check(f"{label} on {grid}, P = {P}", x, h, _ref(label), _CASES[label][1])


@pytest.mark.parametrize("option", mc.OPTIONS)
@pytest.mark.parametrize("grid,P", mc.OPTION_GRIDS)
def test_options(lsfc, identity, grid, P, option):
    M = identity(grid, P)
    label = mc.option_label(M.N, option)
    x, h = _run(lsfc, M, label)
    _check(f"{label}, P = {P}", x, h, _ref(label), _CASES[label][1])
    if option == "cap":
        assert not h.isconverged and mc.CAP <= h.mvps <= mc.CAP + 4 and "max_mv_products" in h.message
    else:
        assert h.isconverged


# -- 2: one rank is the single-device solve, bit for bit -----------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 2])
def test_one_rank_is_the_single_device_solve(lsfc, identity, l):
    grid = (16, 16, 16)
    label = mc.grouped_label(16 ** 3, l)
    x, h = _run(lsfc, identity(grid, 1), label)
    x1, h1 = _run(lsfc, identity(grid, None), label)
    assert h.iters > 3 and (h.iters, h.mvps, h.isconverged) == (h1.iters, h1.mvps, h1.isconverged)
    assert np.array_equal(h["resnorm"], h1["resnorm"]), (h["resnorm"], h1["resnorm"])
    assert np.array_equal(x.view(np.float64), x1.view(np.float64))


# -- 3: two solves of the same input are bitwise equal -------------------------------------------------------------------------
def test_repeated_solves_are_bitwise_equal(lsfc, identity):
    M = identity((16, 16, 16), 4)
    for l in (1, 2, 4):
        label = mc.grouped_label(M.N, l)
        x0, h0 = _run(lsfc, M, label)
        x1, h1 = _run(lsfc, M, label)
        assert h0.iters > 3 and np.array_equal(h0["resnorm"], h1["resnorm"]) and np.array_equal(x0.view(np.float64), x1.view(np.float64)), l


# -- 4: the real operator --------------------------------------------------------------------------------------------------------
_REAL = {}


def _real_reference(name):
    """(A, rhs of the plane wave, the fp64 restatement, its true residual) through the oracle's apply_reduced, computed once"""
    if name not in _REAL:
        c = cases.case_3d(name)
        Mo, n = c["M"], c["n"]
        G2 = o.reduce_symbol(Mo.GFFT, (n, n, n))
        A = lambda v: o.apply_reduced(G2, Mo.nu, Mo.omega, v, (n, n, n))       # noqa: E731
        u_inc = cases.plane_wave(c["k"], c["X"])
        rhs = -(A(u_inc) - u_inc)
        ref = br.bicgstabl_ref(rhs, a=A, l=2, reltol=1e-10, dtype=np.complex128)
        _REAL[name] = (A, rhs, ref, float(np.linalg.norm(A(ref["x"]) - rhs) / np.linalg.norm(rhs)))
    return _REAL[name]


@pytest.mark.parametrize("name,P", [("gv16k10", 4), ("gv32k10", 8)])
def test_real_operator(lsfc, name, P):
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    c = cases.case_3d(name)
    Mo, n = c["M"], c["n"]
    N = n ** 3
    A, rhs, ref, res_ref = _real_reference(name)
    M = MultiDeviceFastM3D(n, c["h"], c["k"], Mo.nu, devices=[0] * P)
    try:
        u, h = lsfc.bicgstabl_multi_(np.zeros(N, complex), M, rhs, l=2, reltol=1e-10, log=True)
        res = float(np.linalg.norm(A(u) - rhs) / np.linalg.norm(rhs))
        print(f"{name}, P = {P}: device {h.iters} cycles, true residual {res:.3e}; fp64 restatement {ref['iters']} cycles, {res_ref:.3e}")
        assert ref["converged"] and h.isconverged
        assert res <= 10 * res_ref
        assert abs(h.iters - ref["iters"]) <= 1
        # the host preconditioner of the multi-device GMRES test, on the whole vector
        d = 1.0 + Mo.omega ** 2 * 0.01 * Mo.nu
        calls = []
        u, h = lsfc.bicgstabl_multi_(np.zeros(N, complex), M, rhs, l=2, Pl=_scale_by(1.0 / d, calls), reltol=1e-10, log=True)
        assert len(calls) == h.mvps > 0 and set(calls) == {N}       # one call for the initial residual, one per application
        tol = 1e-10 * np.linalg.norm(rhs / d)
        res = float(np.linalg.norm((A(u) - rhs) / d))
        print(f"{name}, P = {P}, preconditioned: {h.iters} cycles, true preconditioned residual {res / tol:.3f} tol")
        assert h.isconverged and res <= 2 * tol
    finally:
        M.close()


# -- 5: breakdown -----------------------------------------------------------------------------------------------------------------
def test_breakdown_keeps_the_last_finite_iterate(lsfc, identity):
    # the construction of tests/test_gpu_bicgstabl.py on the grid: a shadow residual orthogonal to the residual, rho == 0, then
    # sigma == <r~, Pl A us[0]> == 0 in the first BiCG step of cycle 1 -- every rank forms that sigma from the same rank sums,
    # so every rank skips the updates of the cycle and x stays x0 bit for bit
    L = lsfc._lib
    grid, N = (16, 16, 16), 16 ** 3
    lam = np.where(np.arange(N) % 2 == 0, 1.0, 2.0).astype(complex)
    b, shadow, x0 = np.zeros(N, complex), np.zeros(N, complex), np.zeros(N, complex)
    b[0], shadow[1], x0[0] = 1.0, 1.0, 0.25
    ref = br.bicgstabl_ref(b, pl=lam, l=1, r_shadow=shadow, x0=x0, max_mv_products=10)
    assert ref["breakdown"] == "sigma" and not ref["converged"] and ref["iters"] == 1
    kw = dict(l=1, Pl=_scale_by(lam), r_shadow=shadow, max_mv_products=10, log=True)
    Mm = identity(grid, 4)
    x, h = lsfc.bicgstabl_multi_(x0.copy(), Mm, b, **kw)
    x1, h1 = lsfc.bicgstabl_(x0.copy(), identity(grid, None), b, **kw)
    # the C return code and message, the callback in ctypes
    def scale(user, v, n):
        np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(2 * n,)).view(np.complex128).__imul__(lam)
        return 0
    cb = L.PRECOND_FN(scale)
    xc, res = x0.copy(), L.GmresResult()
    opts = L.BicgstablOpts(l=1, max_mv_products=10, reltol=-1.0, r_shadow=shadow.ctypes.data_as(C.c_void_p))
    opts.precond, opts.precond_on_device = cb, 0
    rc = L.load().lsfc_bicgstabl_multi(Mm._plan, xc.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0,
                                 C.byref(res), L.LSFC_MEM_HOST)
    msg = L.load().lsfc_last_error().decode()
    assert not h.isconverged and (h.iters, h.mvps) == (ref["iters"], ref["mvps"]) == (1, 3)
    assert np.all(np.isfinite(x)) and np.array_equal(x, x0) and np.array_equal(xc, x0)
    assert np.array_equal(h["resnorm"], [0.75])                                     # ||lam (b - x0)||, exact in double
    assert "breakdown in cycle 1" in h.message and "sigma" in h.message
    assert rc == L.LSFC_ENOTCONV and "breakdown in cycle 1" in msg and "sigma" in msg and res.converged == 0
    # ... and what the single-device solve reports for the same input
    assert np.array_equal(x, x1) and np.array_equal(h["resnorm"], h1["resnorm"])
    assert (h.iters, h.mvps, h.isconverged, h.message) == (h1.iters, h1.mvps, h1.isconverged, h1.message)


# -- 6: errors --------------------------------------------------------------------------------------------------------------------
def test_errors(lsfc, identity):
    import torch
    L = lsfc._lib
    M = identity((16, 16, 16), 2)
    N = M.N
    b = br.random_rhs(N, seed=5)
    # device vectors: LSFC_MEM_DEVICE at the C entry point (refused before the pointers are looked at), torch tensors in Python
    x = np.zeros(N, complex)
    res = L.GmresResult()
    opts = L.BicgstablOpts(l=2, reltol=-1.0)
    rc = L.load().lsfc_bicgstabl_multi(M._plan, x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0, C.byref(res),
                                 L.LSFC_MEM_DEVICE)
    assert rc == L.LSFC_EINVAL and b"multi-device plan takes host vectors" in L.load().lsfc_last_error()
    xt = torch.zeros(N, dtype=torch.complex128, device="cuda")
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_multi_(xt, M, torch.from_numpy(b).cuda())
    assert ei.value.code == L.LSFC_EINVAL and "multi-device plan" in str(ei.value) and not torch.any(xt)
    # a preconditioner callback on the device
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_multi_(x, M, b, Pl=lambda v: None, Pl_on_device=True)
    assert ei.value.code == L.LSFC_EINVAL and "multi-device plan takes a host preconditioner callback" in str(ei.value)
    assert not np.any(x)
    # the batched solve
    X = np.zeros((2, N), complex)
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_batch_(X, M, np.array([b, b]))
    assert ei.value.code == L.LSFC_EINVAL and "single-device" in str(ei.value) and "not offered" in str(ei.value) and not np.any(X)
    # each entry point names the other for the plan it does not take
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_(x, M, b)
    assert ei.value.code == L.LSFC_EINVAL and "lsfc_bicgstabl_multi solves" in str(ei.value)
    with pytest.raises(lsfc.LsfcError) as ei:
        lsfc.bicgstabl_multi_(x, identity((16, 16, 16), None), b)
    assert ei.value.code == L.LSFC_EINVAL and "lsfc_bicgstabl solves on a single-device plan" in str(ei.value)
    assert not np.any(x)
