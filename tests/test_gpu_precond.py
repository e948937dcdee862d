"""GPU parity of the device-resident SparsifyingPreconditioner apply (csrc/precond.hip, csrc/trisolve.hip, through the C ABI) against
the oracle's restatement of src/preconditioner.jl:132-170 (host sparse LU), and its use as Pl of the device GMRES.
Tolerance 1e-10 relative l2 on the apply (observed ~1e-14: two sparse triangular solves of a well-conditioned pair)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import cases
import precond_ref as pr
from conftest import rel_err
from fast_solver_lippmann_schwinger_amd.preconditioner import SCHEDULE_FIELDS, _csr_arrays

pytestmark = pytest.mark.gpu


def _pair(n, k=None):
    x, h = cases.grid(n, True)
    k = (0.5 / h) if k is None else k
    X, Y = o.grid2d(x, x)
    nu = o.gaussian_bump(X, Y)
    return cases.sparsifying_pair_2d(n, h, k, nu), (x, h, k, nu)


@pytest.mark.parametrize("n", [9, 33, 101])
def test_apply_matches_host_lu(lsfc, n):
    (Msp, As), _ = _pair(n)
    P = lsfc.SparsifyingPreconditioner(Msp, As)
    Po = o.SparsifyingPreconditioner(Msp, As)
    b = o.random_vector(n * n)
    ref = Po.solve(b)
    v = b.copy()
    P.ldiv_(v)                                            # host vector: staged over PCIe
    assert rel_err(v, ref) < 1e-10
    import torch
    t = torch.from_numpy(b).cuda()
    P.ldiv_(t)                                            # device vector: stays on the device
    torch.cuda.synchronize()
    assert rel_err(t.cpu().numpy(), ref) < 1e-10
    assert np.array_equal(t.cpu().numpy(), v)             # same graph, same arithmetic: bitwise equal
    t2 = torch.from_numpy(ref).cuda()                     # replay on another vector
    P.ldiv_(t2)
    torch.cuda.synchronize()
    assert rel_err(t2.cpu().numpy(), Po.solve(ref)) < 1e-10
    st = P.stats()
    assert st["levels_L"] >= 1 and st["levels_U"] >= 1 and st["launches"] <= st["levels_L"] + st["levels_U"] + 2
    assert rel_err(P.solve(b), ref) < 1e-10 and np.array_equal(b, o.random_vector(n * n))     # out of place leaves b alone


def test_general_lu_with_permutations_and_wide_levels(lsfc):
    # a NON-symmetric matrix made of 500 random 12 x 12 blocks with a few couplings between neighbouring blocks:
    # exercises the row and column permutations of the host LU and dependency levels that are hundreds of rows wide
    # (the multi-workgroup level kernel) next to narrow ones (the single-workgroup chain kernel)
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    nb, bs = 500, 12
    N = nb * bs
    blocks = [rng.standard_normal((bs, bs)) + 1j * rng.standard_normal((bs, bs)) + 6.0 * np.eye(bs) * np.exp(1j * rng.uniform(0, 6.28))
              for _ in range(nb)]
    Msp = sp.block_diag(blocks, format="lil")
    for b_ in range(0, nb - 1, 7):                                 # sparse couplings
        Msp[b_ * bs + 3, (b_ + 1) * bs + 5] = 0.3 - 0.2j
        Msp[(b_ + 1) * bs + 1, b_ * bs + 2] = -0.1 + 0.4j
    Msp = Msp.tocsc()
    As = (sp.random(N, N, density=5.0 / N, random_state=9, format="csr") * (1 + 2j) + sp.identity(N)).tocsr()
    P = lsfc.SparsifyingPreconditioner(Msp, As)
    b = o.random_vector(N)
    assert rel_err(P.solve(b), o.SparsifyingPreconditioner(Msp, As).solve(b)) < 1e-10
    st = P.stats()
    assert st["levels_L"] >= bs - 1 and st["launches"] >= 4


def test_row_scaling_through_the_c_abi(lsfc):
    # Julia's lu(Msp) (UMFPACK) factors a row-scaled matrix, (Rs .* Msp)[p, q] = L U; the C ABI takes Rs as row_scale
    import ctypes as C
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from fast_solver_lippmann_schwinger_amd import _lib as L
    from fast_solver_lippmann_schwinger_amd.preconditioner import _csr_arrays
    (Msp, As), _ = _pair(21)
    N = Msp.shape[0]
    Rs = np.random.default_rng(3).uniform(0.5, 2.0, N)
    lu = spla.splu((sp.diags(Rs) @ Msp).tocsc())
    rg = np.empty(N, np.int64); rg[lu.perm_r] = np.arange(N)
    cs = np.empty(N, np.int64); cs[lu.perm_c] = np.arange(N)
    arrs = [*_csr_arrays(As), *_csr_arrays(lu.L), *_csr_arrays(lu.U), rg, cs, Rs]
    pc = C.c_void_p()
    L.check(L.load().lsfc_precond_create(C.byref(pc), N, *[a.ctypes.data_as(C.c_void_p) for a in arrs], 0))
    b = o.random_vector(N)
    v = b.copy()
    L.check(L.load().lsfc_precond_apply(pc, v.ctypes.data_as(C.c_void_p), 0))
    assert rel_err(v, o.SparsifyingPreconditioner(Msp, As).solve(b)) < 1e-10
    # malformed factors are refused, not solved: an upper entry in L, a permutation with a repeated index
    pc2 = C.c_void_p()
    args = [a.ctypes.data_as(C.c_void_p) for a in arrs]
    args_bad = list(args); args_bad[9] = np.zeros(N, np.int64).ctypes.data_as(C.c_void_p)      # row_gather all zero
    assert L.load().lsfc_precond_create(C.byref(pc2), N, *args_bad, 0) == -1
    Lt = _csr_arrays(lu.U)                                                                      # U passed as "L"
    args_bad = list(args); args_bad[3:6] = [a.ctypes.data_as(C.c_void_p) for a in Lt]
    assert L.load().lsfc_precond_create(C.byref(pc2), N, *args_bad, 0) == -1
    L.load().lsfc_precond_destroy(pc)


def test_argument_errors(lsfc):
    import scipy.sparse as sp
    (Msp, As), _ = _pair(9)
    with pytest.raises(ValueError):
        lsfc.SparsifyingPreconditioner(Msp, sp.identity(80, format="csr"))
    with pytest.raises(NameError):
        lsfc.SparsifyingPreconditioner(Msp, As, solverType="nope")
    P = lsfc.SparsifyingPreconditioner(Msp, As)
    with pytest.raises(ValueError):
        P.ldiv_(np.zeros(5, complex))


def test_gmres_with_device_preconditioner(lsfc):
    # examples/example.jl:85-91 in miniature: gmres!(u, fastconv, rhs, Pl=precond) with the preconditioner applied on
    # the device (no PCIe, no Python in the loop) against the oracle GMRES with the host LU preconditioner
    n = 33
    (Msp, As), (x, h, k, nu) = _pair(n)
    M = lsfc.buildFastConvolution(x, x, h, k, o.gaussian_bump, quadRule="Greengard_Vico")
    Mo = o.build_fast_convolution(x, x, h, k, o.gaussian_bump, quadRule="Greengard_Vico")
    X, Y = o.grid2d(x, x)
    u_inc = np.exp(1j * k * X)
    rhs = -k**2 * o.fft_convolution(Mo, nu * u_inc)
    P = lsfc.SparsifyingPreconditioner(Msp, As)
    Po = o.SparsifyingPreconditioner(Msp, As)
    uo = np.zeros(n * n, complex)
    uo, ho = o.gmres(uo, lambda v: o.fastconvolution(Mo, v), rhs, Pl=Po.solve, restart=20, reltol=1e-8, maxiter=60)
    u = np.zeros(n * n, complex)
    u, hist = lsfc.gmres_(u, M, rhs, Pl=P, restart=20, reltol=1e-8, maxiter=60, log=True)
    assert hist.isconverged == ho.isconverged and abs(hist.iters - ho.iters) <= 1
    m = min(hist.iters, ho.iters)
    ro = np.asarray(ho.resnorm[:m])
    big = ro > 1e3 * 1e-8 * ro[0]
    assert np.max(np.abs(hist["resnorm"][:m] - ro)[big] / ro[big]) < 1e-6
    assert rel_err(u, uo) < 1e-6
    # the same solve with device-resident vectors
    import torch
    ud = torch.zeros(n * n, dtype=torch.complex128, device="cuda")
    ud, hd = lsfc.gmres_(ud, M, torch.from_numpy(rhs).cuda(), Pl=P, restart=20, reltol=1e-8, maxiter=60, log=True)
    assert hd.iters == hist.iters and np.array_equal(ud.cpu().numpy(), u)
    # and it is a useful preconditioner: fewer iterations than without
    u0 = np.zeros(n * n, complex)
    u0, h0 = lsfc.gmres_(u0, M, rhs, restart=20, reltol=1e-8, maxiter=60, log=True)
    print("iterations with / without the sparsifying stand-in:", hist.iters, h0.iters)


# ---- every schedule of the two triangular solves (csrc/trisolve.hip, trisolve_build) against a long-double reference ----
#
# Synthetic factors (tests/precond_ref.py: make_factor) whose dependency levels steer the launch schedule into each of
# its four segment kinds; every recipe is solved as L and, mirrored, as U in the same apply.  Criterion: the device
# result's relative l2 error against the long-double reference is at most 10x that of the same arithmetic in double
# (+ 1e-14), and no entry is off by more than 1e-12 of the largest.  Each case also asserts the schedule counts it
# was built to reach (lsfc_precond_schedule), so a case that stops reaching its kernel fails instead of passing.


def _sched(**kw):
    return tuple(kw.get(f, 0) for f in SCHEDULE_FIELDS)


def _thin(R, rows=1):
    """R rows in consecutive levels of `rows` rows, coupled densely to the 64 rows before them, sparsely to any
    earlier row, or to the 200 rows before them (which reach back before the stretch), with a long row now and then"""
    out = []
    for i in range(R // rows):
        out.append([(rows, 40, 64), (rows, 6), (rows, 25, 200)][i % 3] if i % 50 != 49 else (rows, 300))
    return out


# interleaved 1..16 and 17..32 row levels: 1024, 512, 256, 128, 64 and 32 lanes per row, single-level groups
_CHAIN_A = [lv for r in range(1, 17) for lv in ((r, 20 + 3 * r), (16 + r, 6))]
# multi-level groups, several closing at exactly 16 rows
_CHAIN_B = ([(4, 5)] * 4 + [(20, 5)] + [(8, 30)] * 2 + [(20, 5)] + [(10, 20), (6, 20), (1, 50), (20, 5)]
            + [(1, 30)] * 17 + [(20, 5)] + [(1, 3000), (1, 3000), (20, 5)] + [(2, 7), (5, 9), (3, 11), (6, 13), (20, 5)])
# single-row levels of 2000..8000 entries: all 1024 lanes on one row, folded through LDS over 16 waves
_CHAIN_C = [(1, 2000), (20, 5), (1, 5000), (20, 5), (1, 8000), (20, 5), (1, 4099), (17, 5)]

RECIPES = {
    # kind 0: levels of 300 rows at 8, 16, 32, 64 lanes per row; 33 rows (just over NARROW); one row of 9000 entries
    "level_widths": ([(9100, 0), (300, 4), (300, 15), (300, 30), (300, 60), (33, 5), (1, 9000), (300, 4)],
                     _sched(level8=4, level16=1, level32=1, level64=2)),
    "chains": ([(8200, 0)] + _CHAIN_A + _CHAIN_B + _CHAIN_C, _sched(level8=1, chains=1, chain_groups=6)),
    # heavy groups: 4 single-row levels of 3000 entries between two chains; 2 x 8 rows; one closing a chain segment
    # before a wide level; one closing the factor
    "heavy": ([(12100, 0), (20, 5), (3, 5), (20, 5)] + [(1, 3000)] * 4 + [(17, 5), (20, 5), (2, 5), (20, 5)]
              + [(8, 600)] * 2 + [(20, 5), (1, 4000), (1, 4000), (1, 1000), (300, 4), (20, 5)] + [(1, 3000)] * 3,
              _sched(level8=2, chains=4, heavy_groups=4)),
    # dense runs: R rows of thin levels between two wide levels; 95 stays a chain (6 groups of <= 16 rows)
    **{f"run{R}": ([(400, 0)] + _thin(R) + [(40, 5)],
                   _sched(level8=2, chains=1, chain_groups=6) if R < 96 else
                   _sched(level8=2, run_pieces=(R + 1023) // 1024, run_max=min(R, 1024), run_min=R - 1024 * ((R - 1) // 1024)))
       for R in (95, 96, 127, 128, 129, 1024, 1025)},
    "run1026_3rows": ([(400, 0)] + _thin(1026, 3) + [(40, 5)], _sched(level8=2, run_pieces=2, run_max=1023, run_min=3)),
    "run2100_4rows": ([(400, 0)] + _thin(2100, 4) + [(40, 5)], _sched(level8=2, run_pieces=3, run_max=1024, run_min=52)),
    # every kind in one factor: wide levels, a chain, a run, a chain, a heavy group, a chain
    "mixed": ([(3000, 0), (300, 30), (20, 5), (2, 9), (9, 9)] + _thin(300) + [(20, 5)] + [(1, 3000)] * 3 + [(20, 5), (3, 20), (17, 5)],
              _sched(level8=1, level32=1, chains=3, chain_groups=1, heavy_groups=1, run_pieces=1, run_max=300, run_min=300)),
    # edges: N = 1, N = 2, diagonal only, N = 12345 (tails of the SpMV and scatter launches)
    "n1": ([(1, 0)], _sched(chains=1)),
    "n2": ([(1, 0), (1, 1)], _sched(chains=1, chain_groups=1)),
    "diagonal": ([(500, 0)], _sched(level8=1)),
    "n12345": ([(12000, 0), (300, 8), (45, 20)], _sched(level8=2, level16=1)),
}

TESTS = os.path.dirname(os.path.abspath(__file__))


class _Precond:
    """an lsfc_precond over explicit factors, through the C ABI (None: identity map / unit scale)"""

    def __init__(self, lsfc, As, L, U, rg, cs, rs):
        from fast_solver_lippmann_schwinger_amd import _lib
        self._lib, self.N = _lib, L.shape[0]
        self._keep = [*_csr_arrays(As), *_csr_arrays(L), *_csr_arrays(U),
                      *[None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in ((rg, np.int64), (cs, np.int64), (rs, np.float64))]]
        self._pc = C.c_void_p()
        ptrs = [None if a is None else a.ctypes.data_as(C.c_void_p) for a in self._keep]
        _lib.check(_lib.load().lsfc_precond_create(C.byref(self._pc), self.N, *ptrs, 0))

    def apply(self, b):
        v = np.array(b, dtype=np.complex128)
        self._lib.check(self._lib.load().lsfc_precond_apply(self._pc, v.ctypes.data_as(C.c_void_p), self._lib.LSFC_MEM_HOST))
        return v

    def schedule(self, factor):
        out = (C.c_int64 * len(SCHEDULE_FIELDS))()
        self._lib.check(self._lib.load().lsfc_precond_schedule(self._pc, factor, out))
        return tuple(out)

    def close(self):
        self._lib.load().lsfc_precond_destroy(self._pc)


def _synthetic(name, seed=1):
    """(As, L, U, row_gather, col_scatter, row_scale) of a recipe: L the recipe, U its mirror image; identity As except
    at N = 12345 (a random sparse As), random permutations and row scale"""
    import scipy.sparse as sp
    levels, _ = RECIPES[name]
    L = pr.make_factor(levels, lower=True, seed=seed)
    U = pr.make_factor(levels, lower=False, seed=seed + 100)
    N = L.shape[0]
    rng = np.random.default_rng(seed)
    As = sp.identity(N, dtype=np.complex128, format="csr")
    if N == 12345:
        As = (sp.random(N, N, density=7.0 / N, random_state=seed, format="csr") * (0.3 - 0.1j) + As).tocsr()
    return As, L, U, rng.permutation(N), rng.permutation(N), rng.uniform(0.5, 2.0, N)


def _rhs(N, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


def _assert_matches_reference(v, args, b, what):
    """the accuracy criterion of this section; returns (e_dev, e_f64)"""
    ref = pr.apply_ref(*args, b, np.clongdouble)
    f64 = pr.apply_ref(*args, b, np.complex128)
    nref = np.linalg.norm(ref)
    e_dev = float(np.linalg.norm(v.astype(np.clongdouble) - ref) / nref)
    e_f64 = float(np.linalg.norm(f64.astype(np.clongdouble) - ref) / nref)
    worst = float(np.max(np.abs(v.astype(np.clongdouble) - ref)) / np.max(np.abs(ref)))
    print(f"{what}: rel-l2 device {e_dev:.2e}, double {e_f64:.2e}; max {worst:.2e}")
    assert e_dev <= 10 * e_f64 + 1e-14, (what, e_dev, e_f64)
    assert worst <= 1e-12, (what, worst)
    return e_dev, e_f64


@pytest.mark.parametrize("name", list(RECIPES))
def test_schedule_matches_long_double_reference(lsfc, name):
    args = _synthetic(name)
    P = _Precond(lsfc, *args)
    try:
        sL, sU = P.schedule(0), P.schedule(1)
        print(f"{name} N={P.N}: L {dict(zip(SCHEDULE_FIELDS, sL))}\n{' ' * len(name)} U {dict(zip(SCHEDULE_FIELDS, sU))}")
        expect = RECIPES[name][1]
        assert sL == expect and sU == expect, (sL, sU, expect)
        b = _rhs(P.N)
        _assert_matches_reference(P.apply(b), args, b, name)
    finally:
        P.close()


def test_schedule_argument_errors(lsfc):
    from fast_solver_lippmann_schwinger_amd import _lib
    lib = _lib.load()
    P = _Precond(lsfc, *_synthetic("n2"))
    out = (C.c_int64 * len(SCHEDULE_FIELDS))()
    try:
        for factor in (-1, 2):
            assert lib.lsfc_precond_schedule(P._pc, factor, out) == -1 and b"factor" in lib.lsfc_last_error()
        assert lib.lsfc_precond_schedule(P._pc, 0, None) == -1
        assert lib.lsfc_precond_schedule(None, 0, out) == -1
        assert lib.lsfc_precond_schedule(P._pc, 1, out) == 0 and tuple(out) == RECIPES["n2"][1]
    finally:
        P.close()


def _real_pair(kind, n):
    if kind == "gv3":                                      # the device-built 3D pair, as in test_gpu_sparsify.py
        from test_gpu_sparsify import case
        import fast_solver_lippmann_schwinger_amd as pkg
        M = case("gv3", (n, n, n))[0]
        return pkg.sparsifying_pair(M)
    return _pair(n)[0]


@pytest.mark.parametrize("kind,n", [("gv3", 16), ("gv3", 24), ("2d", 33), ("2d", 101)])
def test_real_factors_match_long_double_reference(lsfc, kind, n):
    import scipy.sparse.linalg as spla
    Msp, As = _real_pair(kind, n)
    lu = spla.splu(Msp.tocsc())
    P = lsfc.SparsifyingPreconditioner(Msp, As, lu=lu)
    N = Msp.shape[0]
    rg = np.empty(N, np.int64)
    rg[lu.perm_r] = np.arange(N)
    cs = np.empty(N, np.int64)
    cs[lu.perm_c] = np.arange(N)
    b = _rhs(N)
    st = P.stats()
    print(f"{kind} n={n}: L {st['schedule_L']}\n{' ' * len(kind)} U {st['schedule_U']}")
    _assert_matches_reference(P.solve(b), (As, lu.L, lu.U, rg, cs, None), b, f"{kind} n={n}")
    if (kind, n) == ("gv3", 24):                           # the real 3D factor reaches heavy groups and several run pieces
        assert st["schedule_U"]["heavy_groups"] > 0 and st["schedule_U"]["run_pieces"] > 1, st["schedule_U"]


def test_3d_preconditioned_residual_history_matches_host_lu(lsfc):
    # with left preconditioning GMRES converges to A^-1 b for any nonsingular Pl; its residual history does depend on Pl.
    # Device GMRES with the device preconditioner against the oracle's GMRES with the host LU of the SAME device-built pair
    import scipy.sparse.linalg as spla
    from test_gpu_sparsify import case
    M, _, _, _, Mo = case("gv3", (24, 24, 24))
    x = -0.5 + np.arange(24) / 24
    u_inc = np.exp(1j * 24.0 * o.grid3d(x, x, x)[0])
    rhs = -(M * u_inc - u_inc)
    Msp, As = lsfc.sparsifying_pair(M)
    lu = spla.splu(Msp.tocsc())
    P = lsfc.SparsifyingPreconditioner(Msp, As, lu=lu)
    tol = 1e-10
    u = np.zeros(rhs.size, complex)
    u, hist = lsfc.gmres_(u, M, rhs, Pl=P, restart=20, reltol=tol, maxiter=60, log=True)
    uo = np.zeros(rhs.size, complex)
    uo, ho = o.gmres(uo, lambda v: o.mul(Mo, v), rhs, Pl=lambda v: lu.solve(As @ v), restart=20, reltol=tol, maxiter=60)
    print(f"3D 24^3, reltol {tol}: {hist.iters} device iterations, {ho.iters} oracle")
    assert hist.isconverged and ho.isconverged and abs(hist.iters - ho.iters) <= 1
    m = min(hist.iters, ho.iters)
    ro = np.asarray(ho.resnorm[:m])
    big = ro > 1e3 * tol * ro[0]
    assert big.sum() >= 3
    assert np.max(np.abs(hist["resnorm"][:m] - ro)[big] / ro[big]) < 1e-6


def test_graph_replay_and_stream_launches_are_bitwise_equal(lsfc, tmp_path):
    # LSFC_PRECOND_GRAPH is read once per process: the launches without the graph run in a fresh child process
    assert os.environ.get("LSFC_PRECOND_GRAPH", "1")[:1] != "0", "this process must replay the captured graph"
    args = _synthetic("mixed")
    P = _Precond(lsfc, *args)
    try:
        b = _rhs(P.N)
        v = P.apply(b)
    finally:
        P.close()
    _assert_matches_reference(v, args, b, "mixed, graph")
    out = tmp_path / "nograph.npy"
    script = "\n".join([
        "import sys", f"sys.path[:0] = [{TESTS!r}, {os.path.dirname(TESTS)!r}]",
        "import numpy as np", "import fast_solver_lippmann_schwinger_amd as pkg",
        "from test_gpu_precond import _Precond, _synthetic, _rhs",
        "P = _Precond(pkg, *_synthetic('mixed'))", f"np.save({str(out)!r}, P.apply(_rhs(P.N)))", "P.close()"])
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, LSFC_PRECOND_GRAPH="0"), capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert np.array_equal(np.load(out), v)


def test_apply_on_a_side_stream_waits_for_the_writer(lsfc):
    # v is written by a kernel on a torch side stream that starts late; the apply enqueued right after it on that stream
    # (ldiv_ follows torch's current stream) must read the written v, not what was there before
    import torch
    import scipy.sparse.linalg as spla
    (Msp, As), _ = _pair(33)
    lu = spla.splu(Msp.tocsc())
    P = lsfc.SparsifyingPreconditioner(Msp, As, lu=lu)
    N = Msp.shape[0]
    rg = np.empty(N, np.int64)
    rg[lu.perm_r] = np.arange(N)
    cs = np.empty(N, np.int64)
    cs[lu.perm_c] = np.arange(N)
    b = _rhs(N)
    src = torch.from_numpy(b).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        v = torch.zeros_like(src)
        torch.cuda._sleep(50_000_000)                     # the writer is late
        v.mul_(0).add_(src)                               # the kernel that writes v
        P.ldiv_(v)
    s.synchronize()
    _assert_matches_reference(v.cpu().numpy(), (As, lu.L, lu.U, rg, cs, None), b, "side stream")
