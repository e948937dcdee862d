"""GPU tests of the device preconditioner with its Schur inverses stored in single precision (csrc/blocktri_factor.hip, csrc/blocktri_sweep.hip,
LSFC_PRECOND_INV_F32; `inverse_dtype="complex64"`): the factorisation is the fp64 one, every S_k^{-1} is rounded once to an
interleaved float pair when it is stored, and the sweeps widen on load and sum in fp64.

References: the fp64 object of the same input (its blocks cast to complex64 are what must be stored, bit for bit), the
numpy restatement of the sweeps on the fetched blocks (tests/blocktri_ref.py; bound 1e-12, only the fp64 summation order
differs), the restatement with its own blocks rounded to complex64 (how far the float object may sit from the fp64 one),
and GMRES with the fp64 object (at most one more inner step)."""
import ctypes as C
import re
import time

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import blocktri_ref as bt
from conftest import rel_err
from test_gpu_sparsify import case, E2E, nu3
from test_gpu_precond_blocktri import CASES

pytestmark = pytest.mark.gpu

FLOAT_MIN_NORMAL = float(np.finfo(np.float32).tiny)        # 1.18e-38
SQRT_EPS = np.sqrt(np.finfo(float).eps)
RELTOL = 1e-6                                              # of the GMRES runs of tests/test_gpu_precond_blocktri.py


def _nblocks(dims):
    return dims[1] if dims[2] == 1 else dims[2]


def _columns(N, nrhs, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nrhs, N)) + 1j * rng.standard_normal((nrhs, N))


_BUILT = {}


def _objects(lsfc, kind, dims):
    """(P64, P32, Msp, As) of a case, built once per session"""
    if (kind, dims) not in _BUILT:
        Msp, As = lsfc.sparsifying_pair(case(kind, dims)[0])
        K = _nblocks(dims)
        P64 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K)
        P32 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K, inverse_dtype="complex64")
        _BUILT[(kind, dims)] = (P64, P32, Msp, As)
    return _BUILT[(kind, dims)]


def _round(S):
    return S.astype(np.complex64).astype(np.complex128)


@pytest.mark.parametrize("kind,dims", CASES)
def test_stored_blocks_are_the_rounded_fp64_blocks(lsfc, kind, dims):
    P64, P32, _, _ = _objects(lsfc, kind, dims)
    smallest = np.inf
    for k in range(_nblocks(dims)):
        S64, S32 = P64.blocktri_block(k), P32.blocktri_block(k)
        parts = np.abs(np.concatenate([S64.real.ravel(), S64.imag.ravel()]))
        smallest = min(smallest, parts[parts > 0].min())
        assert smallest >= FLOAT_MIN_NORMAL, f"block {k}: a part of {smallest:.2e} would round to a float denormal"
        assert np.array_equal(S32, _round(S64)), f"block {k}"
        assert np.array_equal(S32, _round(S32)), f"block {k} is not representable in complex64"
    print(f"{kind} {dims}: smallest nonzero part of any fp64 S_k^-1 {smallest:.2e}")


@pytest.mark.parametrize("kind,dims", CASES)
def test_info_reports_the_storage(lsfc, kind, dims):
    import fast_solver_lippmann_schwinger_amd._lib as L
    P64, P32, Msp, _ = _objects(lsfc, kind, dims)
    K = _nblocks(dims)
    b = Msp.shape[0] // K
    i64, i32 = P64.blocktri_info(), P32.blocktri_info()
    assert sorted(i32) == sorted(i64)                                        # the same fields
    assert i64["factor_bytes"] == K * b * b * 16 and i32["factor_bytes"] == K * b * b * 8
    assert (i32["blocks"], i32["block_size"], i32["launches"]) == (K, b, i64["launches"])
    assert i32["pivoting"] == 0 and i64["pivoting"] == 0
    assert i32["min_pivot_ratio"] == i64["min_pivot_ratio"]
    assert P64.inverse_dtype == "complex128" and P32.inverse_dtype == "complex64"
    prec = C.c_int(-1)
    assert L.load().lsfc_precond_inverse_precision(P32._pc, C.byref(prec)) == 0 and prec.value == L.LSFC_PRECOND_INV_F32
    assert L.load().lsfc_precond_inverse_precision(P64._pc, C.byref(prec)) == 0 and prec.value == L.LSFC_PRECOND_INV_F64
    assert P32.stats()["factor_bytes"] == K * b * b * 8


@pytest.mark.parametrize("kind,dims", CASES)
def test_apply_matches_the_restatement_on_the_stored_blocks(lsfc, kind, dims):
    # (41, 41) and (33, 33): one launch walks both sweeps (b <= 96); the other cases take a launch per step
    P64, P32, Msp, As = _objects(lsfc, kind, dims)
    K = _nblocks(dims)
    assert P32.blocktri_info()["launches"] == (2 if Msp.shape[0] // K <= 96 else 2 * K)
    v = o.random_vector(Msp.shape[0])
    stored = [P32.blocktri_block(k) for k in range(K)]
    err = rel_err(P32.solve(v), bt.solve(Msp, stored, As @ v))
    print(f"{kind} {dims}: float-storage apply vs the restatement on the stored blocks {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("kind,dims", CASES)
def test_distance_from_the_fp64_object(lsfc, kind, dims):
    P64, P32, Msp, As = _objects(lsfc, kind, dims)
    K = _nblocks(dims)
    v = o.random_vector(Msp.shape[0])
    dist = rel_err(P32.solve(v), P64.solve(v))
    Sinv = bt.eliminate(Msp, K)
    w = As @ v
    cpu = rel_err(bt.solve(Msp, [_round(S) for S in Sinv], w), bt.solve(Msp, Sinv, w))
    print(f"{kind} {dims}: float object vs fp64 object {dist:.3e}; restatement with rounded blocks vs itself {cpu:.3e}")
    assert dist > 0.0
    assert dist <= 4.0 * cpu


@pytest.mark.parametrize("kind,dims", CASES)
def test_group_sweep(lsfc, kind, dims):
    P32 = _objects(lsfc, kind, dims)[1]
    Msp = _objects(lsfc, kind, dims)[2]
    N = Msp.shape[0]
    B = _columns(N, 8)
    single = [P32.solve(b) for b in B]
    before = P32.batch_info()
    for R in (1, 2, 5, 8):
        V = P32.solve_batch(B[:R])
        worst = max(rel_err(V[j], single[j]) for j in range(R))
        print(f"{kind} {dims} R = {R}: worst member vs ldiv_ {worst:.2e}")
        assert worst <= 1e-10                                # the bound of tests/test_gpu_precond_batch.py
    after = P32.batch_info()
    assert after["sweeps"] - before["sweeps"] == 4 and after["vectors"] - before["vectors"] == 16
    assert after["largest_group"] == 8
    # the bits of a member: alone, at position 0 of 2, 4 of 5 and 7 of 8, among different companions each time
    b = o.random_vector(N)
    alone = P32.solve_batch(b[None, :])[0]
    for pos, R, seed in ((0, 2, 11), (4, 5, 12), (7, 8, 13)):
        G = _columns(N, R, seed)
        G[pos] = b
        assert np.array_equal(P32.solve_batch(G)[pos], alone), f"position {pos} of {R}"


def _e2e_rhs(lsfc, kind, dims):
    M, _, nu, k, Mo = case(kind, dims)
    if kind == "trap":
        X = o.grid2d(*(2 * [-0.5 + np.arange(dims[0]) / (dims[0] - 1)]))[0]
        u_inc = np.exp(1j * k * X)
        return M, Mo, -k ** 2 * lsfc.FFTconvolution(M, nu * u_inc)           # examples/example.jl:76-77
    x = -0.5 + np.arange(dims[0]) / dims[0]
    u_inc = np.exp(1j * k * o.grid3d(x, x, x)[0])
    return M, Mo, -(M * u_inc - u_inc)                                        # examples/example3D.jl:71-72


@pytest.mark.parametrize("kind,dims,bound", E2E)
def test_gmres_takes_at_most_one_more_step(lsfc, kind, dims, bound):
    M, _, rhs = _e2e_rhs(lsfc, kind, dims)
    N = rhs.size
    P64, P32, Msp, As = _objects(lsfc, kind, dims)
    u64, h64 = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=P64, reltol=RELTOL, log=True)
    u32, h32 = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=P32, reltol=RELTOL, log=True)
    diff = rel_err(u32, u64)
    true_res = float(np.linalg.norm(M * u32 - rhs) / np.linalg.norm(rhs))
    print(f"{kind} {dims}: {h32.iters} iterations at float storage, {h64.iters} at fp64; solutions differ by {diff:.2e}, "
          f"true residual at float storage {true_res:.2e}")
    assert h32.isconverged and h64.isconverged
    assert h32.iters <= h64.iters + 1
    assert h32.iters <= bound                              # the oracle's count + 1 (tests/test_gpu_sparsify.py)
    assert diff <= 10 * RELTOL


def test_gmres_batch_histories_are_the_solo_histories(lsfc):
    kind, dims = "gv3", (24, 24, 24)
    M, _, nu, k, _ = case(kind, dims)
    x = -0.5 + np.arange(dims[0]) / dims[0]
    X, Y, Z = o.grid3d(x, x, x)
    RHS = np.ascontiguousarray(np.stack([-(M * np.exp(1j * k * d) - np.exp(1j * k * d)) for d in (X, Y, (X + Y + Z) / np.sqrt(3.0))]))
    N = RHS.shape[1]
    P32 = _objects(lsfc, kind, dims)[1]
    sweeps = P32.batch_info()["sweeps"]
    single = [lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, RHS[j], Pl=P32, reltol=RELTOL, log=True) for j in range(3)]
    assert P32.batch_info()["sweeps"] == sweeps            # single solves take the single-vector path
    Xb, hists = lsfc.gmres_batch_(np.zeros_like(RHS), M, RHS, Pl=P32, reltol=RELTOL, log=True)
    assert P32.batch_info()["sweeps"] > sweeps and P32.batch_info()["largest_group"] >= 3
    for j in range(3):
        u, h = single[j]
        r1, rb = np.asarray(h["resnorm"]), np.asarray(hists[j]["resnorm"])
        print(f"member {j}: {hists[j].iters} iterations (alone: {h.iters}), solutions differ by {rel_err(Xb[j], u):.2e}")
        assert hists[j].isconverged and h.isconverged
        assert hists[j].iters == h.iters
        assert np.all(np.abs(rb - r1) <= SQRT_EPS * r1)
        assert rel_err(Xb[j], u) <= 1e-8


def test_determinism_and_routes(lsfc):
    M = case("gv3", (16, 16, 16))[0]
    Msp, As = lsfc.sparsifying_pair(M)
    P1 = lsfc.SparsifyingPreconditioner.from_operator(M, inverse_dtype="complex64")
    P2 = lsfc.SparsifyingPreconditioner.from_operator(M, inverse_dtype="complex64")
    P3 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=16, inverse_dtype="complex64")
    assert P1.inverse_dtype == P2.inverse_dtype == P3.inverse_dtype == "complex64" and P1.Msp is None
    assert lsfc.SparsifyingPreconditioner.from_operator(M).inverse_dtype == "complex128"
    for k in range(16):
        S = P1.blocktri_block(k)
        assert np.array_equal(S, P2.blocktri_block(k)) and np.array_equal(S, P3.blocktri_block(k)), k
    b = o.random_vector(16 ** 3)
    x1 = P1.solve(b)
    assert np.array_equal(x1, P2.solve(b)) and np.array_equal(x1, P3.solve(b)) and np.array_equal(x1, P1.solve(b))
    B = _columns(16 ** 3, 5)
    assert np.array_equal(P1.solve_batch(B), P3.solve_batch(B))


def test_reference_3d_size(lsfc):
    # 48^3 as tests/test_gpu_precond_blocktri.py builds it (examples/example3D.jl)
    import torch
    n = 48
    h = 1.0 / n
    k = 1.0 / h
    x = -0.5 + h * np.arange(n)
    X, Y, Z = o.grid3d(x, x, x)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu3)
    u_inc = np.exp(1j * k * X)
    rhs = -(M * u_inc - u_inc)
    P64 = lsfc.SparsifyingPreconditioner.from_operator(M)
    P32 = lsfc.SparsifyingPreconditioner.from_operator(M, inverse_dtype="complex64")
    i64, i32 = P64.blocktri_info(), P32.blocktri_info()
    assert i32["factor_bytes"] == 48 * 2304 ** 2 * 8 and round(i32["factor_bytes"] / 1e9, 2) == 2.04
    assert i64["factor_bytes"] == 2 * i32["factor_bytes"] and i32["min_pivot_ratio"] == i64["min_pivot_ratio"]
    u64, h64 = lsfc.gmres_(np.zeros(n ** 3, dtype=np.complex128), M, rhs, Pl=P64, reltol=RELTOL, log=True)
    u32, h32 = lsfc.gmres_(np.zeros(n ** 3, dtype=np.complex128), M, rhs, Pl=P32, reltol=RELTOL, log=True)
    res = float(np.linalg.norm(M * u32 - rhs) / np.linalg.norm(rhs))
    print(f"48^3: {h32.iters} iterations at float storage, {h64.iters} at fp64; solutions differ by {rel_err(u32, u64):.2e}, "
          f"true residual {res:.2e}; factorisation {i32['factor_us'] / 1e6:.2f} s (fp64 storage {i64['factor_us'] / 1e6:.2f} s)")
    assert h32.isconverged and h64.isconverged
    assert h32.iters <= h64.iters + 1
    assert rel_err(u32, u64) <= 10 * RELTOL
    assert res <= 1e-5
    vd = torch.from_numpy(o.random_vector(n ** 3)).cuda()

    def median_of_5(P):
        P.ldiv_(vd.clone())                                # warm-up
        times = []
        for _ in range(5):
            w = vd.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            P.ldiv_(w)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return float(np.median(times))

    t64, t32 = median_of_5(P64), median_of_5(P32)
    print(f"48^3: apply {t64 * 1e3:.2f} ms at fp64 storage ({2 * i64['factor_bytes'] / t64 / 1e12:.2f} TB/s), "
          f"{t32 * 1e3:.2f} ms at float storage ({2 * i32['factor_bytes'] / t32 / 1e12:.2f} TB/s)")


def test_error_paths(lsfc):
    import torch
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    rowptr, col, _ = lsfc.sparsify_pattern(9, 9, 1)
    N, nnz = 81, col.size
    rng = np.random.default_rng(0)
    a_val = rng.standard_normal(nnz) + 1j * rng.standard_normal(nnz)
    m_val = a_val.copy()
    m_val[np.repeat(np.arange(N), np.diff(rowptr)) == col] += 20.0
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731

    def create(N_, K_, prec):
        pc = C.c_void_p()
        rc = lib.lsfc_precond_create_blocktri_prec(C.byref(pc), N_, K_, p(rowptr), p(col), p(a_val), p(m_val), L.LSFC_MEM_HOST, 0, prec)
        return rc, pc, lib.lsfc_last_error().decode()

    for bad in (-1, 2, 3):
        rc, pc, msg = create(N, 9, bad)
        assert rc == -1 and not pc.value and "inverse_precision" in msg, msg
    M = case("gv2", (33, 33, 1))[0]
    pc = C.c_void_p()
    assert lib.lsfc_precond_create_from_plan_prec(C.byref(pc), M._plan, 5) == -1 and not pc.value
    # the C constructor at both precisions, and the query
    for prec, per in ((L.LSFC_PRECOND_INV_F64, 16), (L.LSFC_PRECOND_INV_F32, 8)):
        rc, pc, msg = create(N, 9, prec)
        assert rc == 0 and pc.value, msg
        got, out6 = C.c_int(-1), (C.c_int64 * 6)()
        assert lib.lsfc_precond_inverse_precision(pc, C.byref(got)) == 0 and got.value == prec
        assert lib.lsfc_precond_inverse_precision(pc, None) == -1
        assert lib.lsfc_precond_blocktri_info(pc, out6, None) == 0 and out6[2] == 9 * 9 ** 2 * per
        lib.lsfc_precond_destroy(pc)
    # Python argument errors
    Msp, As = lsfc.sparsifying_pair(M)
    with pytest.raises(ValueError, match="inverse_dtype"):
        lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=33, inverse_dtype="float32")
    with pytest.raises(ValueError, match="inverse_dtype"):
        lsfc.SparsifyingPreconditioner.from_operator(M, inverse_dtype="single")
    with pytest.raises(ValueError, match="blocktri"):
        lsfc.SparsifyingPreconditioner(Msp, As, factor="host", inverse_dtype="complex64")
    # an object of the host-LU route keeps no inverses
    Ph = lsfc.SparsifyingPreconditioner(Msp, As)
    got = C.c_int(-1)
    assert lib.lsfc_precond_inverse_precision(Ph._pc, C.byref(got)) == -1 and got.value == -1
    assert Ph.inverse_dtype is None
    # The memory rule, from the dimensions and the precision alone: blocks of 4096 rows, so many that even the float
    # inverses are twice the free memory.  Both requests are refused before an array is read (the arrays here are far too
    # short) or anything is allocated, and the figures of the two messages are the rule at 16 and at 8 bytes per entry.
    free = torch.cuda.mem_get_info()[0]
    b = 4096
    K = int(4 * free // (b * b * 16)) + 1
    figures = {}
    for prec, name in ((L.LSFC_PRECOND_INV_F64, "complex128"), (L.LSFC_PRECOND_INV_F32, "complex64")):
        rc, pc, msg = create(K * b, K, prec)
        print(msg)
        assert rc == -3 and not pc.value and name in msg, msg
        m = re.search(r"need ([0-9.]+) GB for the inverses .* and ([0-9.]+) GB of work space, ([0-9.]+) GB of device memory are free", msg)
        assert m, msg
        figures[name] = tuple(float(g) for g in m.groups())
    inv64, work64, _ = figures["complex128"]
    inv32, work32, _ = figures["complex64"]
    assert abs(inv64 - K * b * b * 16 / 1e9) <= 1e-3 and abs(inv32 - K * b * b * 8 / 1e9) <= 1e-3
    assert inv64 > free / 1e9                              # the fp64 inverses alone do not fit
    assert abs((work32 - work64) - 2 * b * b * 16 / 1e9) <= 2e-3          # two fp64 work blocks more
    assert inv32 + work32 <= inv64 / 2 + work64 + 2 * b * b * 16 / 1e9 + 3e-3
    assert torch.cuda.mem_get_info()[0] >= free - (1 << 28)                 # nothing of that size was allocated
