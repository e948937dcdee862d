"""GPU tests of the preconditioner factorised on the device (csrc/blocktri_factor.hip: lsfc_precond_create_blocktri,
lsfc_precond_create_from_plan): block-tridiagonal elimination of Msp with dense explicit inverses of the Schur blocks.

References: scipy's sparse LU of the same Msp, the numpy restatement of the elimination (tests/blocktri_ref.py) and
numpy.linalg.inv.  Bound 1e-10: the project's parity bar for the preconditioner (tests/test_gpu_precond.py)."""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import lsfc_oracle as o
import blocktri_ref as bt
from conftest import rel_err
from test_gpu_sparsify import case, E2E, nu3

pytestmark = pytest.mark.gpu

CASES = [("trap", (41, 41, 1)), ("trap", (101, 101, 1)), ("gv2", (33, 33, 1)), ("gv3", (16, 16, 16)), ("gv3", (18, 12, 10)),
         ("gv3", (24, 24, 24))]


def _nblocks(dims):
    return dims[1] if dims[2] == 1 else dims[2]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("kind,dims", CASES)
def test_device_factorisation_matches_sparse_lu_and_restatement(lsfc, kind, dims):
    M = case(kind, dims)[0]
    Msp, As = lsfc.sparsifying_pair(M)
    K = _nblocks(dims)
    P = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K)
    b = o.random_vector(Msp.shape[0])
    w = As @ b
    x = P.solve(b)
    xo = spla.splu(Msp.tocsc()).solve(w)
    err, res = rel_err(x, xo), float(np.linalg.norm(Msp @ x - w) / np.linalg.norm(w))
    Sinv = bt.eliminate(Msp, K)
    worst = max(rel_err(P.blocktri_block(k), Sinv[k]) for k in range(K))
    st = P.stats()
    print(f"{kind} {dims}: solve vs splu {err:.2e}, residual {res:.2e}, blocks vs restatement {worst:.2e}, "
          f"min pivot ratio {st['min_pivot_ratio']:.3f}, {st['launches']} launches, factorised in {st['factor_us'] / 1e3:.1f} ms")
    assert err <= 1e-10
    assert res <= 1e-10
    assert worst <= 1e-10
    assert st["blocks"] == K == st["levels_L"] == st["levels_U"] and st["block_size"] == Msp.shape[0] // K
    assert st["factor_bytes"] == K * st["block_size"] ** 2 * 16 and st["pivoting"] == 0


@pytest.mark.parametrize("b", [41, 216, 1000, 2304])
def test_dense_inversion_alone(lsfc, b):
    # nblocks = 1, As = I (stored on the full pattern), Msp = a random complex matrix with a dominant diagonal
    rng = np.random.default_rng(b)
    A = rng.standard_normal((b, b)) + 1j * rng.standard_normal((b, b))
    A[np.arange(b), np.arange(b)] += 4.0 * np.sqrt(b) * np.exp(2j * np.pi * rng.random(b))
    print(f"b = {b}: cond(A) = {np.linalg.cond(A):.1f}")
    P = lsfc.SparsifyingPreconditioner(sp.csr_matrix(A), _full_identity(b), factor="blocktri", nblocks=1)
    inv = np.linalg.inv(A)
    err = rel_err(P.blocktri_block(0), inv)
    v = o.random_vector(b)
    serr = rel_err(P.solve(v), inv @ v)
    print(f"b = {b}: inverse vs numpy.linalg.inv {err:.2e}, solve {serr:.2e}, min pivot ratio {P.stats()['min_pivot_ratio']:.3f}")
    assert err <= 1e-10 and serr <= 1e-10


def _full_identity(b):
    """the identity with every entry of the b x b pattern stored (explicit zeros)"""
    return sp.csr_matrix((np.eye(b, dtype=np.complex128).ravel(), np.tile(np.arange(b), b), np.arange(b + 1) * b), shape=(b, b))


def test_from_operator_is_bitwise_the_two_step_route(lsfc):
    M = case("gv3", (16, 16, 16))[0]
    Msp, As = lsfc.sparsifying_pair(M)
    P1 = lsfc.SparsifyingPreconditioner.from_operator(M)                      # device arrays that never leave the device
    P2 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=16)   # host arrays
    P3 = lsfc.SparsifyingPreconditioner.from_operator(M)
    assert P1.Msp is None and P1.N == 16 ** 3
    b = o.random_vector(16 ** 3)
    x1, x2, x3 = P1.solve(b), P2.solve(b), P3.solve(b)
    assert np.array_equal(x1, x2) and np.array_equal(x1, x3)
    assert np.array_equal(P1.solve(b), x1)                                   # and the apply repeats
    for k in (0, 7, 15):
        assert np.array_equal(P1.blocktri_block(k), P2.blocktri_block(k)) and np.array_equal(P1.blocktri_block(k), P3.blocktri_block(k))


@pytest.mark.parametrize("kind,dims,bound", E2E)
def test_gmres_with_the_device_factorised_preconditioner(lsfc, kind, dims, bound):
    M, _, nu, k, _ = case(kind, dims)
    N = int(np.prod(dims))
    if kind == "trap":
        X = o.grid2d(*(2 * [-0.5 + np.arange(dims[0]) / (dims[0] - 1)]))[0]
        u_inc = np.exp(1j * k * X)
        rhs = -k ** 2 * lsfc.FFTconvolution(M, nu * u_inc)                   # examples/example.jl:76-77
    else:
        x = -0.5 + np.arange(dims[0]) / dims[0]
        u_inc = np.exp(1j * k * o.grid3d(x, x, x)[0])
        rhs = -(M * u_inc - u_inc)                                             # examples/example3D.jl:71-72
    Msp, As = lsfc.sparsifying_pair(M)
    Ph = lsfc.SparsifyingPreconditioner(Msp, As, lu=spla.splu(Msp.tocsc()))
    Pd = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=_nblocks(dims))
    uh, hh = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=Ph, reltol=1e-6, log=True)
    ud, hd = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=Pd, reltol=1e-6, log=True)
    rh, rd = np.asarray(hh["resnorm"]), np.asarray(hd["resnorm"])
    print(f"{kind} {dims}: {hd.iters} iterations (host LU: {hh.iters}), histories differ by "
          f"{np.max(np.abs(rd - rh[:len(rd)]) / rh[:len(rd)]) if len(rd) <= len(rh) else float('nan'):.2e}, solutions by {rel_err(ud, uh):.2e}")
    assert hd.isconverged and hh.isconverged
    assert hd.iters == hh.iters
    assert np.all(np.abs(rd - rh) <= np.sqrt(np.finfo(float).eps) * rh)
    assert rel_err(ud, uh) <= 1e-8


def test_reference_3d_size_is_preconditioned(lsfc):
    # examples/example3D.jl: h = 1/48, k = 1/h, x = -a/2:h:a/2-h, nu of :43, rhs = -(M u_inc - u_inc), gmres! at reltol 1e-6.
    # No host LU here: scipy's splu of this Msp does not finish within minutes.
    n = 48
    h = 1.0 / n
    k = 1.0 / h
    x = -0.5 + h * np.arange(n)
    X, Y, Z = o.grid3d(x, x, x)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu3)
    u_inc = np.exp(1j * k * X)
    rhs = -(M * u_inc - u_inc)
    t0 = time.perf_counter()
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    setup = time.perf_counter() - t0
    u, hist = lsfc.gmres_(np.zeros(n ** 3, dtype=np.complex128), M, rhs, Pl=P, reltol=1e-6, log=True)
    u0, hist0 = lsfc.gmres_(np.zeros(n ** 3, dtype=np.complex128), M, rhs, reltol=1e-6, maxiter=400, log=True)
    res = float(np.linalg.norm(M * u - rhs) / np.linalg.norm(rhs))
    st = P.stats()
    print(f"48^3: {hist.iters} preconditioned iterations, {hist0.iters} without; set-up {setup:.2f} s (factorisation "
          f"{st['factor_us'] / 1e6:.2f} s, {st['factor_bytes'] / 1e9:.2f} GB), true residual {res:.2e}, min pivot ratio {st['min_pivot_ratio']:.3f}")
    assert hist.isconverged
    assert hist.iters < hist0.iters
    assert res <= 1e-5
    assert setup <= 60.0                                   # assembly plus factorisation: the host LU did not finish in 240 s


def test_error_paths(lsfc):
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    rowptr, col, _ = lsfc.sparsify_pattern(9, 9, 1)
    N, nnz = 81, col.size
    rng = np.random.default_rng(0)
    a_val = rng.standard_normal(nnz) + 1j * rng.standard_normal(nnz)
    m_val = a_val.copy()
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    m_val[rows == col] += 20.0

    def create(N_, K_, rp, cl, av, mv):
        pc = C.c_void_p()
        rc = lib.lsfc_precond_create_blocktri(C.byref(pc), N_, K_, _ptr(rp), _ptr(cl), _ptr(av), _ptr(mv), L.LSFC_MEM_HOST, 0)
        return rc, pc, lib.lsfc_last_error().decode()

    rc, pc, _ = create(N, 9, rowptr, col, a_val, m_val)
    assert rc == 0 and pc.value
    out10 = (C.c_int64 * 10)()
    assert lib.lsfc_precond_schedule(pc, 0, out10) == -1                     # no level schedule on this kind of object
    a, b_, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert lib.lsfc_precond_stats(pc, C.byref(a), C.byref(b_), C.byref(c)) == 0 and (a.value, b_.value) == (9, 9) and c.value >= 2
    lib.lsfc_precond_destroy(pc)
    # an entry outside the band: 27 blocks of 3 rows on a 9 x 9 grid
    rc, pc, msg = create(N, 27, rowptr, col, a_val, m_val)
    assert rc == -1 and not pc.value and "row" in msg and "block diagonals" in msg, msg
    # N not divisible by nblocks
    rc, pc, msg = create(N, 10, rowptr, col, a_val, m_val)
    assert rc == -1 and "divisible" in msg, msg
    # NULL pointer
    pcn = C.c_void_p()
    assert lib.lsfc_precond_create_blocktri(C.byref(pcn), N, 9, _ptr(rowptr), _ptr(col), None, _ptr(m_val), L.LSFC_MEM_HOST, 0) == -1
    # a zero row in Msp: a clean error that names block and row, no object (so no NaN is reachable through apply)
    z_val = m_val.copy()
    z_val[rowptr[40]:rowptr[41]] = 0.0
    rc, pc, msg = create(N, 9, rowptr, col, a_val, z_val)
    assert rc != 0 and not pc.value and "block 4" in msg and "row 40" in msg, msg
    # 256^3 is rejected from its dimensions alone (17.6 TB), before any array is read: the arrays here are far too short
    rc, pc, msg = create(256 ** 3, 256, rowptr, col, a_val, m_val)
    assert rc == -3 and not pc.value and "GB" in msg, msg
    print(msg)
    # info / get_block on an object of lsfc_precond_create
    import cases
    n = 17
    hh = 1.0 / (n - 1)
    xx = -0.5 + hh * np.arange(n)
    Xg, Yg = o.grid2d(xx, xx)
    Msp, As = cases.sparsifying_pair_2d(n, hh, 1.0 / hh, 0.3 * np.exp(-40 * (Xg ** 2 + Yg ** 2)))
    Ph = lsfc.SparsifyingPreconditioner(Msp, As)
    out6 = (C.c_int64 * 6)()
    blk = np.empty(n * n, dtype=np.complex128)
    assert lib.lsfc_precond_blocktri_info(Ph._pc, out6, None) == -1
    assert lib.lsfc_precond_blocktri_get_block(Ph._pc, 0, _ptr(blk), blk.size) == -1
    assert "schedule_L" in Ph.stats()                                        # objects of the host route report as before
