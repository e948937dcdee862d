"""GPU tests of the device preconditioner applied to several right-hand sides at once (csrc/blocktri_sweep.hip:
blocktri_enqueue_batch; csrc/precond.hip: lsfc_precond_apply_batch and the one apply sequence; csrc/gmres.hip: the second rendezvous of
lsfc_gmres_batch): groups of up to 8 vectors go through one sweep that reads every S_k^{-1} once.

References: scipy's sparse LU of the same Msp, the numpy restatement of the elimination (tests/blocktri_ref.py) and the
single-vector apply of the same object.  Bound 1e-10: the project's parity bar for the preconditioner."""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from oracle import lsfc_oracle as o
import blocktri_ref as bt
import cases
from conftest import rel_err
from test_gpu_sparsify import case, nu3

pytestmark = pytest.mark.gpu

CASES = [("trap", (41, 41, 1)), ("trap", (101, 101, 1)), ("gv2", (33, 33, 1)), ("gv3", (16, 16, 16)), ("gv3", (18, 12, 10)),
         ("gv3", (24, 24, 24))]
GROUPS = [1, 2, 3, 5, 8, 11]
SQRT_EPS = np.sqrt(np.finfo(float).eps)


def _nblocks(dims):
    return dims[1] if dims[2] == 1 else dims[2]


def _columns(N, nrhs, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nrhs, N)) + 1j * rng.standard_normal((nrhs, N))


_PAIRS = {}


def _pair(lsfc, kind, dims):
    """(Msp, As) of a case, assembled once per session"""
    if (kind, dims) not in _PAIRS:
        _PAIRS[(kind, dims)] = lsfc.sparsifying_pair(case(kind, dims)[0])
    return _PAIRS[(kind, dims)]


def _blocktri(lsfc, kind, dims):
    Msp, As = _pair(lsfc, kind, dims)
    return lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=_nblocks(dims)), Msp, As


@pytest.mark.parametrize("kind,dims", CASES)
def test_every_column_matches_sparse_lu_restatement_and_single_apply(lsfc, kind, dims):
    P, Msp, As = _blocktri(lsfc, kind, dims)
    N = Msp.shape[0]
    B = _columns(N, max(GROUPS))
    lu = spla.splu(Msp.tocsc())
    Sinv = bt.eliminate(Msp, _nblocks(dims))
    x_lu = [lu.solve(As @ b) for b in B]
    x_bt = [bt.solve(Msp, Sinv, As @ b) for b in B]
    x_one = [P.solve(b) for b in B]
    for R in GROUPS:
        V = P.solve_batch(B[:R])
        assert V.shape == (R, N)
        e_lu = max(rel_err(V[j], x_lu[j]) for j in range(R))
        e_bt = max(rel_err(V[j], x_bt[j]) for j in range(R))
        e_one = max(rel_err(V[j], x_one[j]) for j in range(R))
        print(f"{kind} {dims} R = {R}: worst column vs splu {e_lu:.2e}, vs restatement {e_bt:.2e}, vs P.solve {e_one:.2e}")
        assert e_lu <= 1e-10
        assert e_bt <= 1e-10
        assert e_one <= 1e-10


@pytest.mark.parametrize("kind,dims", CASES)
def test_result_does_not_depend_on_the_group(lsfc, kind, dims):
    # the bits of a member's result: alone, at position 0 of 2, 4 of 5 and 7 of 8, among different companions each time
    P, Msp, _ = _blocktri(lsfc, kind, dims)
    N = Msp.shape[0]
    b = o.random_vector(N)
    alone = P.solve_batch(b[None, :])[0]
    for pos, R, seed in ((0, 2, 11), (4, 5, 12), (7, 8, 13)):
        B = _columns(N, R, seed)
        B[pos] = b
        V = P.solve_batch(B)
        assert np.array_equal(V[pos], alone), f"position {pos} of {R}"


@pytest.mark.parametrize("kind,dims", [("trap", (41, 41, 1)), ("gv3", (18, 12, 10)), ("gv3", (24, 24, 24))])
def test_repeatable_across_applies_and_objects(lsfc, kind, dims):
    P1, Msp, _ = _blocktri(lsfc, kind, dims)
    P2 = _blocktri(lsfc, kind, dims)[0]
    B = _columns(Msp.shape[0], 5)
    V1 = P1.solve_batch(B)
    assert np.array_equal(P1.solve_batch(B), V1)
    assert np.array_equal(P2.solve_batch(B), V1)


@pytest.mark.parametrize("kind,dims", [("trap", (41, 41, 1)), ("gv3", (16, 16, 16))])
def test_eleven_vectors_are_two_sweeps(lsfc, kind, dims):
    P, Msp, _ = _blocktri(lsfc, kind, dims)
    assert P.batch_info() == {"sweeps": 0, "vectors": 0, "largest_group": 0, "work_bytes": 0}
    B = _columns(Msp.shape[0], 11)
    V = P.solve_batch(B)
    info = P.batch_info()
    print(f"{kind} {dims}: {info}")
    assert info["sweeps"] == 2 and info["vectors"] == 11 and info["largest_group"] == 8
    assert info["work_bytes"] >= 3 * 8 * Msp.shape[0] * 16
    for j in (0, 7, 8, 10):                                # both groups
        assert rel_err(V[j], P.solve(B[j])) <= 1e-10


@pytest.mark.parametrize("kind,dims", CASES)
def test_single_apply_is_untouched_by_batched_calls(lsfc, kind, dims):
    P, Msp, _ = _blocktri(lsfc, kind, dims)
    b = o.random_vector(Msp.shape[0])
    before = P.solve(b)
    P.solve_batch(_columns(Msp.shape[0], 3))
    assert np.array_equal(P.solve(b), before)


def test_host_lu_object_applies_row_by_row(lsfc):
    Msp, As = _pair(lsfc, "trap", (41, 41, 1))
    Ph = lsfc.SparsifyingPreconditioner(Msp, As)
    B = _columns(Msp.shape[0], 11)
    V = Ph.solve_batch(B)
    for j in range(11):
        assert np.array_equal(V[j], Ph.solve(B[j])), j
    assert Ph.batch_info() == {"sweeps": 0, "vectors": 0, "largest_group": 0, "work_bytes": 0}


def test_torch_device_rows_in_place(lsfc):
    import torch
    P, Msp, _ = _blocktri(lsfc, "gv3", (18, 12, 10))
    B = _columns(Msp.shape[0], 5)
    Vd = torch.from_numpy(B).cuda()
    out = P.ldiv_batch_(Vd)
    torch.cuda.synchronize()
    assert out is Vd
    assert np.array_equal(Vd.cpu().numpy(), P.solve_batch(B))


def _plane_wave_rhs(lsfc, kind, dims):
    """three incident plane waves (along x, along y, along a diagonal), right-hand sides as in
    tests/test_gpu_precond_blocktri.py (examples/example.jl:76-77, examples/example3D.jl:71-72)"""
    M, _, nu, k, _ = case(kind, dims)
    if kind == "trap":
        x = -0.5 + np.arange(dims[0]) / (dims[0] - 1)
        X, Y = o.grid2d(x, x)
        dirs = (X, Y, (X + Y) / np.sqrt(2.0))
        RHS = np.stack([-k ** 2 * lsfc.FFTconvolution(M, nu * np.exp(1j * k * d)) for d in dirs])
    else:
        x = -0.5 + np.arange(dims[0]) / dims[0]
        X, Y, Z = o.grid3d(x, x, x)
        dirs = (X, Y, (X + Y + Z) / np.sqrt(3.0))
        RHS = np.stack([-(M * np.exp(1j * k * d) - np.exp(1j * k * d)) for d in dirs])
    return M, np.ascontiguousarray(RHS)


@pytest.mark.parametrize("kind,dims", [("trap", (101, 101, 1)), ("gv3", (24, 24, 24))])
def test_gmres_batch_meets_at_the_preconditioner(lsfc, kind, dims):
    import torch
    M, RHS = _plane_wave_rhs(lsfc, kind, dims)
    N = RHS.shape[1]
    Msp, As = _pair(lsfc, kind, dims)
    Ps = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=_nblocks(dims))       # the single solves' object
    single = []
    for j in range(3):
        u, h = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, RHS[j], Pl=Ps, reltol=1e-6, log=True)
        single.append((u, h))
    assert Ps.batch_info()["sweeps"] == 0                                    # lsfc_gmres is unchanged

    def check(X, hists, Pd, what):
        info = Pd.batch_info()
        print(f"{kind} {dims} {what}: {info}")
        assert info["largest_group"] == 3 and info["vectors"] > info["sweeps"] > 0
        for j in range(3):
            u, h = single[j]
            r1, rb = np.asarray(h["resnorm"]), np.asarray(hists[j]["resnorm"])
            print(f"  row {j}: {hists[j].iters} iterations (alone: {h.iters}), histories differ by "
                  f"{np.max(np.abs(rb - r1[:len(rb)]) / r1[:len(rb)]) if len(rb) <= len(r1) else float('nan'):.2e}, "
                  f"solutions by {rel_err(X[j], u):.2e}")
            assert hists[j].isconverged and h.isconverged
            assert hists[j].iters == h.iters
            assert np.all(np.abs(rb - r1) <= SQRT_EPS * r1)
            assert rel_err(X[j], u) <= 1e-8

    Pd = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=_nblocks(dims))
    X, hists = lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, Pl=Pd, reltol=1e-6, log=True)
    check(X, hists, Pd, "host arrays")
    Pt = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=_nblocks(dims))
    Xd, hd = lsfc.gmres_batch_(torch.zeros(RHS.shape, dtype=torch.complex128, device="cuda"), M, torch.from_numpy(RHS).cuda(), Pl=Pt,
                               reltol=1e-6, log=True)
    torch.cuda.synchronize()
    check(Xd.cpu().numpy(), hd, Pt, "device tensors")


def test_gmres_batch_with_a_python_callable_is_as_before(lsfc):
    # the comparison of tests/test_gpu_batch.py:113-128 against this build: a host callable keeps the serialised path
    c = cases.case_3d("gv16k10")
    Mo, n, k = c["M"], c["n"], c["k"]
    M = lsfc.buildFastConvolution3D(c["x"], c["x"], c["x"], c["X"], c["Y"], c["Z"], c["h"], k, c["nu"])
    U_inc = np.stack([np.exp(1j * k * c["X"]), np.exp(1j * k * (0.6 * c["Y"] + 0.8 * c["Z"])), 0.01 * np.exp(1j * k * c["Z"])])
    RHS = -(lsfc.apply_batch(M, U_inc, 0) - U_inc)
    d = 1.0 + Mo.omega ** 2 * 0.01 * Mo.nu

    def Pl(v):
        v /= d
    X2 = np.zeros_like(RHS)
    X2, h2 = lsfc.gmres_batch_(X2, M, RHS, Pl=Pl, restart=5, reltol=1e-9, log=True)
    for j in range(3):
        u1 = np.zeros(n ** 3, complex)
        u1, h1 = lsfc.gmres_(u1, M, RHS[j], Pl=Pl, restart=5, reltol=1e-9, log=True)
        assert h2[j].iters == h1.iters and rel_err(X2[j], u1) < 1e-10

    def bad(v):
        raise RuntimeError("boom")
    with pytest.raises(RuntimeError):
        lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, Pl=bad, restart=5)
    M.close()


def test_reference_3d_size_eight_right_hand_sides(lsfc):
    # 48^3 as in test_reference_3d_size_is_preconditioned: 8 right-hand sides through one group sweep against 8 single
    # applies of the same object in the same process (the single apply is the code of before: this only rules out a slowdown)
    import torch
    n = 48
    h = 1.0 / n
    k = 1.0 / h
    x = -0.5 + h * np.arange(n)
    X, Y, Z = o.grid3d(x, x, x)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu3)
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    B = _columns(n ** 3, 8)
    V = P.solve_batch(B)
    errs = [rel_err(V[j], P.solve(B[j])) for j in range(8)]
    print(f"48^3: 8 columns batched vs P.solve, worst {max(errs):.2e}")
    assert max(errs) <= 1e-10
    Bd = torch.from_numpy(B).cuda()

    def batched():
        P.ldiv_batch_(Bd.clone())

    def singles():
        W = Bd.clone()
        for j in range(8):
            P.ldiv_(W[j])

    def median_of_5(fn):
        fn()                                               # warm-up
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return float(np.median(times))

    tb, ts = median_of_5(batched), median_of_5(singles)
    print(f"48^3: 8 right-hand sides batched {tb * 1e3:.2f} ms, 8 single applies {ts * 1e3:.2f} ms, ratio {tb / ts:.3f}; {P.batch_info()}")
    assert tb < ts


def test_error_paths(lsfc):
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    P, Msp, _ = _blocktri(lsfc, "trap", (41, 41, 1))
    N = Msp.shape[0]
    V = _columns(N, 2)
    pv = V.ctypes.data_as(C.c_void_p)
    out4 = (C.c_int64 * 4)()
    assert lib.lsfc_precond_apply_batch(None, pv, 2, L.LSFC_MEM_HOST) == -1
    assert lib.lsfc_precond_apply_batch(P._pc, None, 2, L.LSFC_MEM_HOST) == -1
    assert lib.lsfc_precond_apply_batch(P._pc, pv, 0, L.LSFC_MEM_HOST) == -1 and "nrhs" in lib.lsfc_last_error().decode()
    assert lib.lsfc_precond_apply_batch(P._pc, pv, 2, 7) == -1 and "memspace" in lib.lsfc_last_error().decode()
    assert lib.lsfc_precond_batch_info(None, out4) == -1 and lib.lsfc_precond_batch_info(P._pc, None) == -1
    assert P.batch_info()["sweeps"] == 0                                     # nothing was enqueued by the refused calls
    with pytest.raises(ValueError, match="DimensionMismatch"):
        P.ldiv_batch_(np.zeros((2, N + 1), dtype=np.complex128))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        P.ldiv_batch_(np.zeros(N, dtype=np.complex128))                       # a vector is not a batch
    with pytest.raises(ValueError, match="DimensionMismatch"):
        P.ldiv_batch_(np.zeros((0, N), dtype=np.complex128))
    with pytest.raises(TypeError, match="complex128"):
        P.ldiv_batch_(np.zeros((2, N), dtype=np.complex64))
    with pytest.raises(TypeError, match="contiguous"):
        P.ldiv_batch_(np.zeros((N, 2), dtype=np.complex128).T)
