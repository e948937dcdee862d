"""GPU tests of the block-tridiagonal preconditioner (csrc/blocktri_factor.hip, csrc/blocktri_sweep.hip) at every boundary of its kernel shapes: the
synthetic inputs of tests/blocktri_cases.py (`SHAPES`: block sizes on both sides of each tile constant, patterns that are
no stencils), both storages of the inverses, every group size from 1 to 8.

References: the numpy restatement of the elimination (`blocktri_ref.eliminate`) and scipy's sparse LU, bound 1e-10 (the
project's parity bar for a factorisation against an independent one); the two sweeps in long double on the blocks fetched
from the object (`blocktri_cases.solve_ld`), bound 1e-12 (only the fp64 summation order differs; the reference itself
sits at <= 5e-15, tests/test_blocktri_cases_cpu.py).  Vectors are compared in norm and elementwise
(max|x - ref| <= bound max|ref|), so that one wrong row of 4098 cannot hide in a norm."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import blocktri_ref as bt
import blocktri_cases as bc
from conftest import rel_err

pytestmark = pytest.mark.gpu

FLOAT_MIN_NORMAL = float(np.finfo(np.float32).tiny)        # 1.18e-38
STORAGES = ("complex128", "complex64")

shapes = pytest.mark.parametrize("shape", bc.SHAPES, ids=bc.shape_id)


def _pick(*sizes):
    return pytest.mark.parametrize("shape", [s for s in bc.SHAPES if s[0] in sizes], ids=bc.shape_id)


def _both(x, ref):
    """(normwise, elementwise) error"""
    return rel_err(x, ref), bc.elementwise_err(x, ref)


def _build(lsfc, shape):
    Msp, As, _ = bc.built(shape)
    return {dt: lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=shape[1], inverse_dtype=dt) for dt in STORAGES}


_BUILT = {}


def _objects(lsfc, shape):
    """{storage: object} of a shape, built once per session"""
    if shape not in _BUILT:
        _BUILT[shape] = _build(lsfc, shape)
    return _BUILT[shape]


_FETCHED = {}


def _fetched(lsfc, shape, storage):
    """the blocks of the session's object as stored, fetched once; read only"""
    if (shape, storage) not in _FETCHED:
        P = _objects(lsfc, shape)[storage]
        _FETCHED[(shape, storage)] = [P.blocktri_block(k) for k in range(shape[1])]
    return _FETCHED[(shape, storage)]


@shapes
def test_blocks(lsfc, shape):
    b, K, _ = shape
    Sinv = bc.built(shape)[2]
    P = _objects(lsfc, shape)
    S64, S32 = _fetched(lsfc, shape, "complex128"), _fetched(lsfc, shape, "complex64")
    worst = (0.0, 0.0)
    for k in range(K):
        err = _both(S64[k], Sinv[k])
        worst = max(worst[0], err[0]), max(worst[1], err[1])
        assert err[0] <= 1e-10 and err[1] <= 1e-10, f"block {k}: {err}"
        assert np.array_equal(S32[k], S64[k].astype(np.complex64).astype(np.complex128)), f"block {k}: not the fp64 block cast to float"
    print(f"{bc.shape_id(shape)}: blocks vs the restatement {worst[0]:.2e} in norm, {worst[1]:.2e} elementwise")
    for dt, per in (("complex128", 16), ("complex64", 8)):
        info = P[dt].blocktri_info()
        assert (info["blocks"], info["block_size"], info["factor_bytes"]) == (K, b, K * b * b * per)
        assert info["launches"] == (2 if b <= 96 else 2 * K) and info["pivoting"] == 0
        assert P[dt].inverse_dtype == dt


@shapes
def test_single_apply(lsfc, shape):
    b, K, _ = shape
    Msp, As, _ = bc.built(shape)
    v = bc.right_hand_sides(b * K, 1, seed=3)[0]
    w = As @ v
    for dt in STORAGES:
        x = _objects(lsfc, shape)[dt].solve(v)
        err = _both(x, bc.solve_ld(Msp, _fetched(lsfc, shape, dt), w))
        print(f"{bc.shape_id(shape)} {dt}: apply vs the long-double sweeps on the stored blocks {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
        assert err[0] <= 1e-12 and err[1] <= 1e-12
        if dt == "complex128" and b * K <= 3000:
            err = _both(x, spla.splu(Msp.tocsc()).solve(w))
            print(f"{bc.shape_id(shape)}: apply vs splu {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
            assert err[0] <= 1e-10 and err[1] <= 1e-10


@shapes
def test_group_apply(lsfc, shape):
    b, K, _ = shape
    N = b * K
    Msp, As, _ = bc.built(shape)
    B = bc.right_hand_sides(N, 8)
    W = (As @ B.T).T
    for dt in STORAGES:
        P = _objects(lsfc, shape)[dt]
        ref = bc.solve_ld(Msp, _fetched(lsfc, shape, dt), W)
        single = [P.solve(v) for v in B]
        worst = [0.0, 0.0, 0.0, 0.0]
        for R in range(1, 9):                              # every instantiation of the group product
            V = P.solve_batch(B[:R])
            for j in range(R):
                e = _both(V[j], ref[j]) + _both(V[j], single[j])
                worst = [max(a, c) for a, c in zip(worst, e)]
                assert e[0] <= 1e-12 and e[1] <= 1e-12, f"{dt}: member {j} of {R} vs the long-double sweeps {e[:2]}"
                assert e[2] <= 1e-10 and e[3] <= 1e-10, f"{dt}: member {j} of {R} vs the single apply {e[2:]}"
        print(f"{bc.shape_id(shape)} {dt}: R = 1..8, worst member vs the long-double sweeps {worst[0]:.2e} / {worst[1]:.2e}, "
              f"vs the single apply {worst[2]:.2e} / {worst[3]:.2e} (norm / elementwise)")
        # the bits of a member: alone, at position 0 of 2, 4 of 5 and 7 of 8, among different companions each time
        v = bc.right_hand_sides(N, 1, seed=5)[0]
        alone = P.solve_batch(v[None, :])[0]
        for pos, R, seed in ((0, 2, 11), (4, 5, 12), (7, 8, 13)):
            G = bc.right_hand_sides(N, R, seed)
            G[pos] = v
            assert np.array_equal(P.solve_batch(G)[pos], alone), f"{dt}: position {pos} of {R}"


@_pick(33, 64, 257, 1025)
def test_repeatable(lsfc, shape):
    # (64, dense): a column of U holds 64 entries whose slots the counter handed out in arbitrary order
    b, K, _ = shape
    first, second = _objects(lsfc, shape), _build(lsfc, shape)
    B = bc.right_hand_sides(b * K, 3)
    for dt in STORAGES:
        for k in range(K):
            assert np.array_equal(second[dt].blocktri_block(k), _fetched(lsfc, shape, dt)[k]), f"{dt}: block {k}"
        x = first[dt].solve(B[0])
        assert np.array_equal(second[dt].solve(B[0]), x) and np.array_equal(first[dt].solve(B[0]), x), dt
        assert np.array_equal(second[dt].solve_batch(B), first[dt].solve_batch(B)), dt


@pytest.mark.parametrize("shape", [s for s in bc.SHAPES if s[0] <= 257], ids=bc.shape_id)
def test_min_pivot_ratio(lsfc, shape):
    P = _objects(lsfc, shape)
    expect = bc.min_pivot_ratio(bc.built(shape)[0], shape[1])
    got = P["complex128"].stats()["min_pivot_ratio"]
    print(f"{bc.shape_id(shape)}: min_pivot_ratio {got:.15e}, Gauss-Jordan without pivoting on the host {expect:.15e}")
    assert abs(got - expect) <= 1e-10 * expect
    assert P["complex64"].stats()["min_pivot_ratio"] == got


# ---- planted pivots -----------------------------------------------------------------------------------------------------

PLANT_B, PLANT_K, PLANT_SMAX = 70, 3, 50.0


def _planted(eps, second=False):
    """(Msp, As), 3 blocks of 70 rows.  U_0 is empty, so S_1 = D_1 exactly; D_1 = smax I except rows and columns 45, 46,
    which hold smax [[eps, 1], [1, eps]]: Gauss-Jordan without pivoting meets the pivot eps smax at row 45 of block 1
    (second 32-column panel), max|S_1| = smax.  `second`: row 3 of block 2 keeps only a diagonal of 1e-12."""
    b, K = PLANT_B, PLANT_K
    Msp, As = bc.synth(b, K, "scattered", seed=45)
    stored = Msp.toarray() != 0                            # the shared pattern as a mask (no stored value is zero)
    Md, Ad = Msp.toarray(), As.toarray()
    stored[:b, b:2 * b] = False                            # U_0 is empty
    one = slice(b, 2 * b)
    stored[one, one] = np.eye(b, dtype=bool)
    stored[[b + 45, b + 46], [b + 46, b + 45]] = True
    Md[one, one] = PLANT_SMAX * np.eye(b)
    Md[b + 45:b + 47, b + 45:b + 47] = PLANT_SMAX * np.array([[eps, 1.0], [1.0, eps]])
    rng = np.random.default_rng(46)
    Ad[one, one] = rng.standard_normal((b, b)) + 1j * rng.standard_normal((b, b))
    if second:
        Md[2 * b + 3, :] = 0.0                             # stored zeros: the pattern stays the shared one
        Md[2 * b + 3, 2 * b + 3] = 1e-12
    rows, cols = np.nonzero(stored)                        # row by row, columns ascending
    indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
    csr = lambda A: sp.csr_matrix((A[rows, cols], cols.astype(np.int64), indptr.copy()), shape=A.shape)   # noqa: E731
    return csr(Md), csr(Ad)


def _create(lsfc, Msp, As, K, prec=None):
    """the C constructor on host arrays: (return code, object or None, message)"""
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    rowptr, col = np.ascontiguousarray(Msp.indptr, dtype=np.int64), np.ascontiguousarray(Msp.indices, dtype=np.int64)
    a_val, m_val = np.ascontiguousarray(As.data, dtype=np.complex128), np.ascontiguousarray(Msp.data, dtype=np.complex128)
    pc = C.c_void_p()
    rc = lib.lsfc_precond_create_blocktri_prec(C.byref(pc), Msp.shape[0], K, p(rowptr), p(col), p(a_val), p(m_val), L.LSFC_MEM_HOST, 0,
                                               L.LSFC_PRECOND_INV_F64 if prec is None else prec)
    msg = lib.lsfc_last_error().decode()
    if rc != 0 or not pc.value:
        return rc, None, msg
    P = lsfc.SparsifyingPreconditioner.__new__(lsfc.SparsifyingPreconditioner)   # as from_operator wraps its handle
    P._pc, P.Msp, P.As, P.solverType, P.factor, P.N = pc, None, None, "UMFPACK", "blocktri", Msp.shape[0]
    return rc, P, msg


def test_planted_pivots(lsfc):
    b, K = PLANT_B, PLANT_K
    # the inputs do what the docstring of _planted says (host)
    for eps in (1e-9, 1e-6):
        Msp, As = _planted(eps)
        assert np.array_equal(Msp.indices, As.indices) and bt.in_band(Msp.indptr, Msp.indices, K)
        S = bc.schur_blocks(Msp, K)
        assert np.array_equal(S[1], Msp[b:2 * b, b:2 * b].toarray()) and np.abs(S[1]).max() == PLANT_SMAX
        ratios = [bt.gauss_jordan_nopivot(Sk)[1] for Sk in S]
        assert abs(ratios[1] - eps) <= 1e-12 * eps and min(ratios[0], ratios[2]) >= 1e-2, ratios
    # eps = 1e-9: breakdown in block 1 at row 45 of the block, no object
    Msp, As = _planted(1e-9)
    rc, P, msg = _create(lsfc, Msp, As, K)
    print(msg)
    assert rc != 0 and P is None
    assert "block 1 " in msg and "row 115 " in msg and "row 45 of the block" in msg, msg
    ratio = float(re.search(r"= ([0-9.eE+-]+) is below", msg).group(1))
    assert abs(ratio - 1e-9) <= 1e-2 * 1e-9, msg
    # a second bad pivot in block 2, row 3: the first one is the one reported
    Msp2, As2 = _planted(1e-9, second=True)
    assert bt.gauss_jordan_nopivot(bc.schur_blocks(Msp2, K)[2][:4, :4])[1] < 1e-12
    rc, P, msg2 = _create(lsfc, Msp2, As2, K)
    print(msg2)
    assert rc != 0 and P is None
    assert "block 1 " in msg2 and "row 115 " in msg2 and "row 45 of the block" in msg2, msg2
    # eps = 1e-6 is above the threshold: an object, and the monitor reports the planted pivot
    Msp, As = _planted(1e-6)
    rc, P, msg = _create(lsfc, Msp, As, K)
    assert rc == 0 and P is not None, msg
    got = P.stats()["min_pivot_ratio"]
    print(f"planted 1e-6: min_pivot_ratio {got:.9e}")
    assert abs(got - 1e-6) <= 1e-6 * 1e-6
    # its solve against the same elimination on the host, inverses by Gauss-Jordan without pivoting: both lose u / eps in
    # the 2 x 2 and differ in the summation order alone
    v = bc.right_hand_sides(b * K, 1, seed=9)[0]
    w = As @ v
    blk = bt._blocks(Msp, K)[1]
    Sinv = []
    for k in range(K):
        Sk = blk(k, k).toarray()
        if k:
            Sk = Sk - blk(k, k - 1) @ (Sinv[-1] @ blk(k - 1, k).toarray())
        Sinv.append(bt.gauss_jordan_nopivot(Sk)[0])
    res = lambda x: float(np.linalg.norm(Msp @ x - w) / np.linalg.norm(w))   # noqa: E731
    r_dev, r_host = res(P.solve(v)), res(bt.solve(Msp, Sinv, w))
    print(f"planted 1e-6: residual of the device solve {r_dev:.3e}, of the host solve without pivoting {r_host:.3e}")
    assert r_dev <= 100.0 * r_host
    P.close()


# ---- float denormals ------------------------------------------------------------------------------------------------------

def _denormal_pair(scale):
    """synth "scattered" (b = 40, K = 2) with Msp and As scaled by `scale` and the rows of Msp scaled by factors between 1e-3
    and 1e3 (a diagonal matrix from the left, so every row stays dominant and no block needs pivoting)"""
    Msp, As = bc.synth(40, 2, "scattered", seed=40)
    rng = np.random.default_rng(41)
    rows = 10.0 ** rng.uniform(-3.0, 3.0, 80)
    per_entry = np.repeat(scale * rows, np.diff(Msp.indptr))
    return (sp.csr_matrix((per_entry * Msp.data, Msp.indices, Msp.indptr), shape=Msp.shape),
            sp.csr_matrix((scale * As.data, As.indices, As.indptr), shape=As.shape))


# 1e40: the parts of S_k^{-1} run from 5e-53 to 2e-39, every one a float denormal or a value that rounds to zero;
# 1e37: from 5e-50 to 2e-36, normal floats next to denormals in one 16-byte load
@pytest.mark.parametrize("scale,normals", [(1e40, False), (1e37, True)])
def test_float_denormals(lsfc, scale, normals):
    b, K = 40, 2
    Msp, As = _denormal_pair(scale)
    assert np.array_equal(Msp.indices, As.indices) and np.array_equal(Msp.indptr, As.indptr)
    # the inputs (host): pivots far above the threshold 1e-8, and parts of the exact blocks below the smallest normal float,
    # down to what rounds to zero
    assert bc.min_pivot_ratio(Msp, K) >= 1e-7
    parts = np.abs(np.concatenate([np.concatenate([S.real.ravel(), S.imag.ravel()]) for S in bt.eliminate(Msp, K)]))
    as_float = parts.astype(np.float32)
    counts = (int(np.sum(parts >= FLOAT_MIN_NORMAL)), int(np.sum((parts > 0) & (parts < FLOAT_MIN_NORMAL))),
              int(np.sum((as_float > 0) & (as_float < FLOAT_MIN_NORMAL))), int(np.sum((parts > 0) & (as_float == 0))))
    print(f"scale {scale:.0e}: parts of the restatement's blocks: {counts[0]} normal floats, {counts[1]} in (0, 1.18e-38), of which "
          f"{counts[2]} round to a denormal and {counts[3]} to zero; range {parts[parts > 0].min():.1e} to {parts.max():.1e}")
    assert min(counts[1:]) >= 100 and (counts[0] >= 100 if normals else counts[0] == 0)
    P64 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K)
    P32 = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=K, inverse_dtype="complex64")
    stored = [P32.blocktri_block(k) for k in range(K)]
    for k in range(K):
        S64 = P64.blocktri_block(k)
        want = S64.astype(np.complex64)                    # IEEE round to nearest even, denormals included
        tiny = (np.abs(want.real) < FLOAT_MIN_NORMAL) & (want.real != 0)
        assert tiny.sum() >= 50                            # the device's own blocks reach the denormal range as well
        bad = stored[k] != want.astype(np.complex128)
        assert not bad.any(), (f"block {k}: {bad.sum()} stored entries are not the fp64 entries cast to float, e.g. "
                               f"{S64[bad][:3]} stored as {stored[k][bad][:3]}")
    B = bc.right_hand_sides(b * K, 3)
    ref = bc.solve_ld(Msp, stored, (As @ B.T).T)
    for name, X in (("single", np.stack([P32.solve(v) for v in B])), ("group of 3", P32.solve_batch(B))):
        for j in range(3):
            err = _both(X[j], ref[j])
            print(f"float denormals, {name}, member {j}: vs the long-double sweeps on the stored blocks {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
            assert err[0] <= 1e-12 and err[1] <= 1e-12
