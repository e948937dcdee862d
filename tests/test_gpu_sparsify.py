"""GPU tests of the sparsifying-matrix assembly on the device (csrc/sparsify.hip, lsfc_sparsify_build) against the
numpy/scipy restatement of the reference (tests/sparsify_ref.py: np.linalg.svd of the explicit rows, COO -> CSC).

The singular vector of each class is defined up to a unit complex factor, so values are compared after aligning the
phase of every row (the product fixes it, include/lsfc.h; the restatement keeps numpy's).  Tolerances: 1e-9 relative
per class on As, AG, Msp; 1e-9 of sigma_max on the singular values."""
import ctypes as C

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import sparsify_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu


def nu2(X, Y):                                             # examples/example.jl:48
    return 0.3 * np.exp(-40 * (X ** 2 + Y ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48)


def nu3(X, Y, Z):                                          # examples/example3D.jl:43
    return 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48)


def case(kind, dims, k=None):
    """(device operator, restatement rows, nu, k, oracle operator or None)"""
    import fast_solver_lippmann_schwinger_amd as pkg
    n = dims[0]
    if kind == "trap":                                     # examples/example.jl: x = -a/2:h:a/2, k = 1/h, D0 = D[1]
        h = 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        k = 1.0 / h if k is None else k
        X, Y = o.grid2d(x, x)
        D0 = o.reference_vals_trap_rule()[1][0]
        M = pkg.buildFastConvolution(x, x, h, k, nu2, quadRule="trapezoidal")
        Mo = o.build_fast_convolution(x, x, h, k, nu2, quadRule="trapezoidal")
        return M, ref.direct_rows(k, X, Y, D0, h), nu2(X, Y), k, Mo
    if kind == "gv2":
        h = 1.0 / n
        x = -0.5 + h * np.arange(n)
        k = 10.0 if k is None else k
        M = pkg.buildFastConvolution(x, x, h, k, nu2, quadRule="Greengard_Vico")
        Mo = o.build_fast_convolution(x, x, h, k, nu2, quadRule="Greengard_Vico")
        X, Y = o.grid2d(x, x)
        return M, ref.conv_rows(Mo), nu2(X, Y), k, Mo
    n, m, l = dims                                         # examples/example3D.jl: x = -a/2:h:a/2-h, k = 1/h
    h = 1.0 / n
    x, y, z = (-0.5 + h * np.arange(v) for v in (n, m, l))
    k = 1.0 / h if k is None else k
    X, Y, Z = o.grid3d(x, y, z)
    M = pkg.buildFastConvolution3D(x, y, z, X, Y, Z, h, k, nu3)
    box = abs(x[-1] - x[0]) + h
    Mo = o.build_fast_convolution3d(x, x, x, X, Y, Z, h, k, nu3) if n == m == l and n % 2 == 0 else None
    return M, ref.gv3d_rows(n, m, l, box, k), nu3(X, Y, Z), k, Mo


def _row_phase(dev, rf, rowptr):
    """per-row unit factor p with dev * p ~ rf"""
    N = rowptr.size - 1
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    s = np.bincount(rows, weights=(np.conj(dev) * rf).real, minlength=N) + 1j * np.bincount(rows, weights=(np.conj(dev) * rf).imag, minlength=N)
    return (s / np.abs(s))[rows]


def _csr(A):
    A = A.tocsr()
    A.sort_indices()
    return A


PARITY = [("trap", (21, 21, 1)), ("trap", (41, 41, 1)), ("gv2", (33, 33, 1)), ("gv3", (16, 16, 16)), ("gv3", (24, 24, 24)),
          ("gv3", (18, 12, 10))]            # non-cube; GV plans need even axes (odd centres: 18/2 = 9)


@pytest.mark.parametrize("kind,dims", PARITY)
def test_device_build_matches_restatement(lsfc, kind, dims):
    M, rows, nu, k, _ = case(kind, dims)
    n, m, l = dims
    d = lsfc.sparsify_arrays(M)
    r = ref.build(rows, n, m, l, nu=nu, k=k)
    As, AG, Msp = _csr(r["As"]), _csr(r["AG"]), _csr(r["Msp"])
    assert np.array_equal(d["rowptr"], As.indptr) and np.array_equal(d["col"], As.indices)
    ph = _row_phase(d["As"], As.data, d["rowptr"])
    rows_of = np.repeat(np.arange(n * m * l), np.diff(d["rowptr"]))
    cls = r["row_class"][rows_of]
    for c in range(r["sigma"].shape[0]):
        sel = cls == c
        for name, rv in (("As", As.data), ("AG", AG.data), ("Msp", Msp.data)):
            err = rel_err(d[name][sel] * ph[sel], rv[sel])
            assert err <= 1e-9, (name, c, err)
    smax = r["sigma"][:, :1]
    assert np.all(np.abs(d["sigma"] - r["sigma"]) <= 1e-9 * smax), np.abs(d["sigma"] - r["sigma"]) / smax
    # the phase convention: the largest entry of each stencil is real and positive
    for c in range(r["sigma"].shape[0]):
        row = int(np.flatnonzero(r["row_class"] == c)[0])
        v = d["As"][d["rowptr"][row]:d["rowptr"][row + 1]]
        top = v[np.argmax(np.abs(v))]
        assert top.imag == 0.0 and top.real > 0, (c, top)
    print(f"{kind} {dims}: sigma_min/sigma_max {(r['sigma'][:, 2] / r['sigma'][:, 0]).min():.2e} .. "
          f"{(r['sigma'][:, 2] / r['sigma'][:, 0]).max():.2e}, sigma_-2/sigma_-1 >= {(r['sigma'][:, 1] / r['sigma'][:, 2]).min():.2f}")


def test_preconditioner_from_device_pair_matches_restatement(lsfc):
    M, rows, nu, k, _ = case("trap", (41, 41, 1))
    Msp, As = lsfc.sparsifying_pair(M)
    r = ref.build(rows, 41, 41, nu=nu, k=k)
    P = lsfc.SparsifyingPreconditioner(Msp, As)
    Po = o.SparsifyingPreconditioner(r["Msp"], r["As"])
    b = o.random_vector(41 * 41)
    assert rel_err(P.solve(b), Po.solve(b)) <= 1e-9


# end to end, the solves of the example drivers (reltol 1e-6, gmres! defaults otherwise).  Iteration counts of the
# restatement's preconditioner with the oracle's GMRES on the CPU: 2D n=101 (k = 100): 4 preconditioned against
# 10 unpreconditioned; 3D n=24 (k = 24): 4 against 6.  Bound: that count + 1.
E2E = [("trap", (101, 101, 1), 5), ("gv3", (24, 24, 24), 5)]


@pytest.mark.parametrize("kind,dims,bound", E2E)
def test_preconditioned_solve_end_to_end(lsfc, kind, dims, bound):
    import scipy.sparse.linalg as spla
    M, rows, nu, k, Mo = case(kind, dims)
    N = int(np.prod(dims))
    if kind == "trap":
        X = o.grid2d(*(2 * [-0.5 + np.arange(dims[0]) / (dims[0] - 1)]))[0]
        u_inc = np.exp(1j * k * X)
        rhs = -k ** 2 * lsfc.FFTconvolution(M, nu * u_inc)                   # examples/example.jl:76-77
    else:
        x = -0.5 + np.arange(dims[0]) / dims[0]
        X = o.grid3d(x, x, x)[0]
        u_inc = np.exp(1j * k * X)
        rhs = -(M * u_inc - u_inc)                                             # examples/example3D.jl:71-72
    Msp, As = lsfc.sparsifying_pair(M)
    P = lsfc.SparsifyingPreconditioner(Msp, As, lu=spla.splu(Msp.tocsc()))
    u = np.zeros(N, dtype=np.complex128)
    u, hist = lsfc.gmres_(u, M, rhs, Pl=P, reltol=1e-6, log=True)
    u0 = np.zeros(N, dtype=np.complex128)
    u0, hist0 = lsfc.gmres_(u0, M, rhs, reltol=1e-6, maxiter=400, log=True)
    print(f"{kind} {dims}: {hist.iters} preconditioned iterations, {hist0.iters} without")
    assert hist.isconverged and hist.iters <= bound and hist.iters < hist0.iters, (hist.iters, hist0.iters)
    # the oracle's preconditioned gmres with the restatement's pair
    r = ref.build(rows, *dims, nu=nu, k=k)
    Po = o.SparsifyingPreconditioner(r["Msp"], r["As"])
    uo = np.zeros(N, dtype=np.complex128)
    uo, _ = o.gmres(uo, lambda v: o.mul(Mo, v), rhs, Pl=Po.solve, reltol=1e-6)
    assert rel_err(u, uo) <= 1e-8


def test_device_memspace_and_repeat_are_bitwise_equal(lsfc):
    import torch
    import fast_solver_lippmann_schwinger_amd._lib as L
    M, _, _, _, _ = case("gv3", (16, 16, 16))
    a = lsfc.sparsify_arrays(M)
    b = lsfc.sparsify_arrays(M)
    for name in ("rowptr", "col", "As", "AG", "Msp", "sigma"):
        assert np.array_equal(a[name], b[name]), name
    N, nnz = a["rowptr"].size - 1, a["col"].size
    t = dict(rowptr=torch.empty(N + 1, dtype=torch.int64, device="cuda"), col=torch.empty(nnz, dtype=torch.int64, device="cuda"),
             As=torch.empty(nnz, dtype=torch.complex128, device="cuda"), AG=torch.empty(nnz, dtype=torch.complex128, device="cuda"),
             Msp=torch.empty(nnz, dtype=torch.complex128, device="cuda"), sigma=torch.empty((27, 3), dtype=torch.float64, device="cuda"))
    p = {kk: C.c_void_p(v.data_ptr()) for kk, v in t.items()}
    L.check(L.load().lsfc_sparsify_build(M._plan, p["rowptr"], p["col"], p["As"], p["AG"], p["Msp"], p["sigma"], L.LSFC_MEM_DEVICE))
    torch.cuda.synchronize()
    for name in ("rowptr", "col", "As", "AG", "Msp", "sigma"):
        assert np.array_equal(t[name].cpu().numpy(), a[name]), name


def test_error_paths(lsfc):
    import torch
    import fast_solver_lippmann_schwinger_amd._lib as L
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    lib = L.load()

    def err(rc):
        assert rc == -1, rc
        return lib.lsfc_last_error().decode()
    assert "NULL plan" in err(lib.lsfc_sparsify_build(None, None, None, None, None, None, None, L.LSFC_MEM_HOST))
    h = 1.0 / 16
    x = -0.5 + h * np.arange(16)
    Me = lsfc.buildFastConvolution(x, x, h, 10.0, nu2, quadRule="Greengard_Vico")          # even 2D grid
    assert "odd" in err(lib.lsfc_sparsify_build(Me._plan, None, None, None, None, None, None, L.LSFC_MEM_HOST))
    Mo = o.build_fast_convolution3d(x, x, x, *o.grid3d(x, x, x), h, 10.0, nu3)
    Mm = MultiDeviceFastM3D(16, h, 10.0, Mo.nu, devices=[0, 0])
    assert "multi-device" in err(lib.lsfc_sparsify_build(Mm._plan, None, None, None, None, None, None, L.LSFC_MEM_HOST))
    M, _, _, _, _ = case("gv3", (16, 16, 16))
    sig_dev = torch.empty((27, 3), dtype=torch.float64, device="cuda")
    assert "sigma" in err(lib.lsfc_sparsify_build(M._plan, None, None, None, None, None, C.c_void_p(sig_dev.data_ptr()), L.LSFC_MEM_HOST))
    sig_host = np.empty((27, 3))
    assert "sigma" in err(lib.lsfc_sparsify_build(M._plan, None, None, None, None, None, sig_host.ctypes.data_as(C.c_void_p),
                                                  L.LSFC_MEM_DEVICE))
    val_host = np.empty(10, dtype=np.complex128)
    assert "As_val" in err(lib.lsfc_sparsify_build(M._plan, None, None, val_host.ctypes.data_as(C.c_void_p), None, None, None,
                                                   L.LSFC_MEM_DEVICE))
    with pytest.raises(ValueError):
        lsfc.buildSparseA3DConv(M.omega * 2, None, None, None, M, 16, 16, 16)
    # the reference-named entry points return the same matrices as the raw call
    As = lsfc.buildSparseA3DConv(M.omega, None, None, None, M, 16, 16, 16)
    a = lsfc.sparsify_arrays(M, ("As",))
    assert np.array_equal(_csr(As).data, a["As"])
