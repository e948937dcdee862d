"""GPU tests of the transposed and the adjoint device preconditioner (lsfc_precond_set_op, P.T, P.H): the transposed sweeps
of csrc/blocktri_sweep.hip on the stored S_k^{-1}, single and in groups, at both storages of the inverses.

References and bounds are those of tests/test_gpu_blocktri_shapes.py for the N apply (the arithmetic is the same sums in
another order): the transposed sweeps in long double on the blocks fetched from the object
(`blocktri_transpose_ref.solve_t_ld`, then As.T), 1e-12 in norm and elementwise; scipy's LU of Msp.T, 1e-10; a group member
against the single apply, 1e-10.  The physical cases are gv3 (16,16,16) and trap (41,41,1) of tests/test_gpu_sparsify.py,
whose GMRES step counts tests/test_blocktri_transpose_cpu.py reproduces from the oracle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import blocktri_cases as bc
import blocktri_transpose_ref as btt
import test_gpu_blocktri_shapes as gs
import test_gpu_sparsify as gsp
from conftest import rel_err

pytestmark = pytest.mark.gpu

STORAGES = gs.STORAGES

# the subset of blocktri_cases.SHAPES that the issue names ...
_NAMED = {(1, 5), (17, 3), (64, 3), (65, 3), (96, 3), (97, 3), (98, 3), (129, 2), (257, 2), (70, 2), (1025, 2), (2049, 2)}
SUBSET = [s for s in bc.SHAPES if s[:2] in _NAMED]
# ... and one shape on each side of every tile constant of the transposed kernels (csrc/blocktri_sweep.hip)
LOCAL = [
    (4, 3, "scattered"), (5, 3, "scattered"),              # WT_COLS = 4: columns in flight per wave of the walk kernel
    (32, 3, "scattered"), (33, 3, "scattered"),            # ST_WAVES * WT_COLS = 32: columns per pass of the walk kernel
    (112, 2, "scattered"), (113, 2, "scattered"),          # ST_COLS = 16: columns (in flight) per workgroup of the step kernel
    (127, 2, "scattered"), (128, 2, "scattered"),          # 128 rows per float wave load; bt_range_t = 128 rows per group
                                                           # workgroup; 4 waves x bt_wcols_t = 32 columns per group tile
                                                           # (129 is in the subset; 64 / 65, the complex-double wave load, too)
    (512, 2, "scattered"), (513, 2, "scattered"),          # ST_WAVES * 64 = 512 rows: second row chunk of a wave, complex double
    (1023, 2, "scattered"), (1024, 2, "scattered"),        # the same at float storage, 1024 rows (1025 is in the subset)
    (2047, 2, "scattered"), (2048, 2, "scattered"),        # bt_range_t 128 -> 256 rows and bt_wcols_t 8 -> 16 columns per wave
                                                           # at 2048; AP_CHUNK: one staging chunk exactly (2049 is in the subset)
]
ALL = SUBSET + [s for s in LOCAL if s not in SUBSET]
shapes = pytest.mark.parametrize("shape", ALL, ids=bc.shape_id)

_both = gs._both


def _objects(lsfc, shape):
    return gs._objects(lsfc, shape)                        # shared with the N suite: built once per session


def _ref_t(lsfc, shape, storage, V):
    """As.T Msp^{-T} V in long double on the blocks the object stores"""
    Msp, As, _ = bc.built(shape)
    return btt.precond_t(Msp, As, gs._fetched(lsfc, shape, storage), V)


@shapes
def test_single_apply(lsfc, shape):
    b, K, _ = shape
    Msp, As, _ = bc.built(shape)
    v = bc.right_hand_sides(b * K, 1, seed=3)[0]
    for dt in STORAGES:
        P = _objects(lsfc, shape)[dt]
        before = P.solve(v)
        x = P.T.solve(v)
        err = _both(x, _ref_t(lsfc, shape, dt, v))
        print(f"{bc.shape_id(shape)} {dt}: P.T vs the long-double transposed sweeps on the stored blocks {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
        assert err[0] <= 1e-12 and err[1] <= 1e-12
        if dt == "complex128" and b * K <= 3000:
            err = _both(x, As.T @ spla.splu(Msp.T.tocsc()).solve(v))
            print(f"{bc.shape_id(shape)}: P.T vs As.T splu(Msp.T) {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
            assert err[0] <= 1e-10 and err[1] <= 1e-10
        assert np.array_equal(P.H.solve(v), np.conj(P.T.solve(np.conj(v)))), f"{dt}: P.H is not conj . P.T . conj"
        assert np.array_equal(P.T.solve(v), x), f"{dt}: a second P.T apply differs"
        assert np.array_equal(P.solve(v), before), f"{dt}: the N apply changed after a transposed one"
        assert _get_op(lsfc, P)[0] == 0


@shapes
def test_group_apply(lsfc, shape):
    b, K, _ = shape
    N = b * K
    B = bc.right_hand_sides(N, 11)
    for dt in STORAGES:
        P = _objects(lsfc, shape)[dt]
        ref = _ref_t(lsfc, shape, dt, B)
        single = [P.T.solve(v) for v in B]
        worst = [0.0, 0.0, 0.0, 0.0]
        for R in list(range(1, 9)) + [11]:                 # every instantiation of the group product; 11: groups of 8 + 3
            V = P.T.solve_batch(B[:R])
            for j in range(R):
                e = _both(V[j], ref[j]) + _both(V[j], single[j])
                worst = [max(a, c) for a, c in zip(worst, e)]
                assert e[0] <= 1e-12 and e[1] <= 1e-12, f"{dt}: member {j} of {R} vs the long-double sweeps {e[:2]}"
                assert e[2] <= 1e-10 and e[3] <= 1e-10, f"{dt}: member {j} of {R} vs the single apply {e[2:]}"
        print(f"{bc.shape_id(shape)} {dt}: R = 1..8, 11, worst member vs the long-double sweeps {worst[0]:.2e} / {worst[1]:.2e}, "
              f"vs the single apply {worst[2]:.2e} / {worst[3]:.2e} (norm / elementwise)")
        # the adjoint of a group is the conjugated transposed group, bit for bit
        assert np.array_equal(P.H.solve_batch(B[:3]), np.conj(P.T.solve_batch(np.conj(B[:3])))), dt
        # the bits of a member: alone, at position 0 of 2, 4 of 5 and 7 of 8, among different companions each time
        v = bc.right_hand_sides(N, 1, seed=5)[0]
        alone = P.T.solve_batch(v[None, :])[0]
        for pos, R, seed in ((0, 2, 11), (4, 5, 12), (7, 8, 13)):
            G = bc.right_hand_sides(N, R, seed)
            G[pos] = v
            assert np.array_equal(P.T.solve_batch(G)[pos], alone), f"{dt}: position {pos} of {R}"


@pytest.mark.parametrize("shape", [s for s in SUBSET if s[0] in (64, 257, 1025)], ids=bc.shape_id)
def test_repeatable(lsfc, shape):
    # (64, dense): a row of the transpose holds 192 entries whose slots the counters handed out in arbitrary order
    b, K, _ = shape
    first, second = _objects(lsfc, shape), gs._build(lsfc, shape)
    B = bc.right_hand_sides(b * K, 3)
    for dt in STORAGES:
        x = first[dt].T.solve(B[0])
        assert np.array_equal(second[dt].T.solve(B[0]), x), dt
        assert np.array_equal(second[dt].T.solve_batch(B), first[dt].T.solve_batch(B)), dt
        assert np.array_equal(second[dt].H.solve(B[1]), first[dt].H.solve(B[1])), dt
    for P in second.values():
        P.close()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------

def _get_op(lsfc, P):
    L = lsfc._lib
    op, nbytes = C.c_int(-1), C.c_int64(-1)
    L.check(L.load().lsfc_precond_get_op(P._pc, C.byref(op), C.byref(nbytes)))
    return op.value, nbytes.value


# the smallest shape of the walk kernels (b <= 96) and the first of the step kernels
@pytest.mark.parametrize("shape", [min(s for s in bc.SHAPES if s[0] <= 96), (97, 3, "scattered")], ids=bc.shape_id)
def test_one_object_through_every_captured_sequence(lsfc, shape):
    """One object replays the single apply and groups of 2 and 8 under N, T, H and N again, the group work space growing
    under T (which drops the group graphs and keeps those of the single apply): every result is bitwise that of the same
    call on a fresh object that has seen nothing else."""
    L = lsfc._lib
    lib = L.load()
    b, K, _ = shape
    Msp, As, _ = bc.built(shape)
    B = bc.right_hand_sides(b * K, 8, seed=9)

    def fresh():
        return lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K)

    def call(P, R):                                        # R = 0: the single apply
        return P.solve(B[0]) if R == 0 else P.solve_batch(B[:R])

    steps = [(L.LSFC_OP_N, 0), (L.LSFC_OP_N, 2), (L.LSFC_OP_T, 8), (L.LSFC_OP_T, 0), (L.LSFC_OP_H, 2), (L.LSFC_OP_N, 0), (L.LSFC_OP_N, 8)]
    P = fresh()
    try:
        for i, (op, R) in enumerate(steps):
            L.check(lib.lsfc_precond_set_op(P._pc, op))
            got = call(P, R)
            Q = fresh()
            try:
                L.check(lib.lsfc_precond_set_op(Q._pc, op))
                assert np.array_equal(got, call(Q, R)), f"step {i}: op {op}, {'single apply' if R == 0 else f'group of {R}'}"
            finally:
                Q.close()
        assert P.batch_info()["largest_group"] == 8 and _get_op(lsfc, P)[0] == L.LSFC_OP_N
    finally:
        P.close()


def _bb_cols(b):                                           # columns per workgroup of the N group product (csrc/blocktri_sweep.hip)
    return 32 if b < 1024 else (64 if b < 2048 else 128)


@pytest.mark.parametrize("shape", [(17, 3, "scattered"), (129, 2, "scattered")], ids=bc.shape_id)
def test_op_state_and_an_object_under_n_only(lsfc, shape):
    L = lsfc._lib
    lib = L.load()
    b, K, _ = shape
    N = b * K
    Msp, As, _ = bc.built(shape)
    P = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K)
    try:
        assert _get_op(lsfc, P) == (0, 0)
        B = bc.right_hand_sides(N, 3)
        P.solve(B[0])
        P.solve_batch(B)
        # used under N only: what the object reported before the transposed apply existed
        assert _get_op(lsfc, P) == (0, 0)
        assert P.blocktri_info()["launches"] == (2 if b <= 96 else 2 * K)
        nranges = -(-b // _bb_cols(b))
        assert P.batch_info() == {"sweeps": 1, "vectors": 3, "largest_group": 3, "work_bytes": 16 * (3 * 3 * N + 3 * b + nranges * 3 * b)}
        # the op is state of the object
        L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_T))
        op, nbytes = _get_op(lsfc, P)
        nnz = Msp.nnz
        assert op == L.LSFC_OP_T and nbytes == 8 * (N + 1) + 2 * 8 * N + 4 * nnz + 2 * 16 * nnz
        v = B[0].copy()
        L.check(lib.lsfc_precond_apply(P._pc, v.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
        L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_H))
        assert _get_op(lsfc, P) == (L.LSFC_OP_H, nbytes)
        L.check(lib.lsfc_precond_get_op(P._pc, C.byref(C.c_int(0)), None))      # table_bytes may be NULL
        L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_N))
        assert _get_op(lsfc, P) == (0, nbytes)
        assert np.array_equal(v, P.T.solve(B[0]))
        # everything else keeps describing the N object
        assert P.blocktri_info()["launches"] == (2 if b <= 96 else 2 * K)
        assert P.stats()["levels_L"] == K and P.inverse_dtype == "complex128"
    finally:
        P.close()


def test_refusals(lsfc):
    import krylov_common as kc
    L = lsfc._lib
    lib = L.load()
    assert lib.lsfc_precond_set_op(None, L.LSFC_OP_T) == L.LSFC_EINVAL
    assert lib.lsfc_precond_get_op(None, C.byref(C.c_int(0)), None) == L.LSFC_EINVAL
    shape = (17, 3, "scattered")
    P = _objects(lsfc, shape)["complex128"]
    for op in (3, -1):
        assert lib.lsfc_precond_set_op(P._pc, op) == L.LSFC_EINVAL and "op" in lib.lsfc_last_error().decode()
    assert _get_op(lsfc, P)[0] == 0
    host = kc._diag_precond(lsfc, np.ones(12, complex))    # an object of lsfc_precond_create (host LU factors)
    try:
        for op in (L.LSFC_OP_T, L.LSFC_OP_H):
            assert lib.lsfc_precond_set_op(host._pc, op) == L.LSFC_EINVAL
            assert "block-tridiagonal" in lib.lsfc_last_error().decode()
        L.check(lib.lsfc_precond_set_op(host._pc, L.LSFC_OP_N))
        assert _get_op(lsfc, host) == (0, 0)
        for make in (lambda: host.T, lambda: host.H):
            with pytest.raises(ValueError):
                make()
    finally:
        host.close()


# ---- the physical cases ---------------------------------------------------------------------------------------------------

_CASES = {}


def _physical(lsfc, case):
    """(operator, preconditioner from the plan, right-hand side, oracle step counts) of a physical case, once per session"""
    if case not in _CASES:
        kind, dims = case
        M, _, _, k, _ = gsp.case(kind, dims)
        n = dims[0]
        h = 1.0 / n if kind == "gv3" else 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        X = (gsp.o.grid3d(x, x, x) if kind == "gv3" else gsp.o.grid2d(x, x))[0]
        u_inc = np.exp(1j * k * X).ravel()
        rhs = -(M * u_inc - u_inc)
        counts, rhs_oracle = btt.oracle_solves(kind, dims)
        assert rel_err(rhs, rhs_oracle) <= 1e-10
        _CASES[case] = M, lsfc.SparsifyingPreconditioner.from_operator(M), rhs, counts
    return _CASES[case]


physical = pytest.mark.parametrize("case", sorted(btt.PHYSICAL), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")


@physical
@pytest.mark.parametrize("which", ["T", "H"])
def test_gmres_on_the_transposed_and_the_adjoint_operator(lsfc, case, which):
    M, P, rhs, counts = _physical(lsfc, case)
    A, Pl = (M.T, P.T) if which == "T" else (M.H, P.H)
    u, hist = lsfc.gmres_(np.zeros(M.N, complex), A, rhs, Pl=Pl, reltol=1e-6, restart=20, log=True)
    u0, hist0 = lsfc.gmres_(np.zeros(M.N, complex), A, rhs, reltol=1e-6, restart=20, maxiter=400, log=True)
    res = float(np.linalg.norm(A * u - rhs) / np.linalg.norm(rhs))
    print(f"{case} M.{which}: {hist.iters} steps with P.{which}, {hist0.iters} without (oracle {counts[which]}), true residual {res:.2e}")
    assert hist.isconverged and hist0.isconverged
    assert hist.iters < hist0.iters
    assert (hist.iters, hist0.iters) == counts[which]
    assert res <= 1e-5
    assert _get_op(lsfc, P)[0] == 0                        # restored after the solve


@physical
def test_bicgstabl_and_the_batch_solvers_on_the_adjoint(lsfc, case):
    M, P, rhs, _ = _physical(lsfc, case)
    A, Pl = M.H, P.H
    u, hist = lsfc.bicgstabl_(np.zeros(M.N, complex), A, rhs, Pl=Pl, reltol=1e-6, log=True)
    res = float(np.linalg.norm(A * u - rhs) / np.linalg.norm(rhs))
    print(f"{case}: bicgstabl on M.H with P.H: {hist.mvps} operator applies, true residual {res:.2e}")
    assert hist.isconverged and res <= 1e-5
    rng = np.random.default_rng(17)
    B = np.stack([rhs, 1j * rhs[::-1], rhs * np.exp(2j * np.pi * rng.random(M.N))])
    for solver, single, kw in ((lsfc.gmres_batch_, lsfc.gmres_, {"restart": 20}), (lsfc.bicgstabl_batch_, lsfc.bicgstabl_, {})):
        before = P.batch_info()
        X, hists = solver(np.zeros((3, M.N), complex), A, B, Pl=Pl, reltol=1e-6, log=True, **kw)
        after = P.batch_info()
        assert all(hj.isconverged for hj in hists)
        # the members met in the transposed group sweeps instead of going one by one
        assert after["sweeps"] > before["sweeps"] and after["vectors"] - before["vectors"] > after["sweeps"] - before["sweeps"]
        assert after["largest_group"] == 3
        for j in range(3):
            xj = single(np.zeros(M.N, complex), A, B[j], Pl=Pl, reltol=1e-6, **kw)
            err = rel_err(X[j], xj)
            print(f"{case} {solver.__name__} member {j}: vs its single solve {err:.2e}")
            assert err <= 1e-10
    assert _get_op(lsfc, P)[0] == 0


def test_solver_gate_at_the_c_entry_points(lsfc):
    """lsfc_gmres and lsfc_bicgstabl accept the library's own object iff its op is the plan's; both directions of a mismatch"""
    L = lsfc._lib
    lib = L.load()
    M, P, rhs, _ = _physical(lsfc, ("trap", (41, 41, 1)))
    x = np.zeros(M.N, complex)
    res = L.GmresResult()

    def gmres():
        opts = L.GmresOpts()
        opts.restart, opts.reltol = 20, 1e-6
        opts.precond = C.cast(lib.lsfc_precond_callback, L.PRECOND_FN)
        opts.precond_user, opts.precond_on_device = P._pc, 1
        x[:] = 0
        return lib.lsfc_gmres(M._plan, x.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p), C.byref(opts), None, 0, C.byref(res), L.LSFC_MEM_HOST)

    def bicg():
        bo = L.BicgstablOpts(l=2, reltol=1e-6)
        bo.precond = C.cast(lib.lsfc_precond_callback, L.PRECOND_FN)
        bo.precond_user, bo.precond_on_device = P._pc, 1
        x[:] = 0
        return lib.lsfc_bicgstabl(M._plan, x.ctypes.data_as(C.c_void_p), rhs.ctypes.data_as(C.c_void_p), C.byref(bo), None, 0, C.byref(res), L.LSFC_MEM_HOST)

    P.set_stream(0)
    L.check(lib.lsfc_plan_set_stream(M._plan, None))
    try:
        for plan_op, pc_op in ((0, 1), (0, 2), (1, 0), (2, 0), (1, 2), (2, 1)):
            L.check(lib.lsfc_plan_set_op(M._plan, plan_op))
            L.check(lib.lsfc_precond_set_op(P._pc, pc_op))
            for call in (gmres, bicg):
                rc = call()
                msg = lib.lsfc_last_error().decode()
                names = ("LSFC_OP_N", "LSFC_OP_T", "LSFC_OP_H")
                assert rc == L.LSFC_EINVAL and "preconditioner" in msg and names[plan_op] in msg and names[pc_op] in msg, (plan_op, pc_op, rc, msg)
        for op in (0, 1, 2):
            L.check(lib.lsfc_plan_set_op(M._plan, op))
            L.check(lib.lsfc_precond_set_op(P._pc, op))
            for call in (gmres, bicg):
                assert call() == 0 and res.converged == 1, (op, call.__name__, lib.lsfc_last_error().decode())
    finally:
        L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N))
        L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_N))
