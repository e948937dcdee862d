"""GPU tests of partial row pivoting inside the Schur blocks of the block-tridiagonal preconditioner (csrc/blocktri_factor.hip:
k_bt_pivot_panel, k_bt_swap_rows, k_bt_unscramble; lsfc_precond_create_blocktri_opts).

Inputs (tests/blocktri_pivot_ref.py): the planted 2 x 2 of the shape suite, synthetic pairs with every block row permuted
(S'_k = Pi_k S_k: condition 2 to 3, and Gauss-Jordan without pivoting breaks down on them), a first column of equal
moduli, and a block with two identical rows.

Bounds, as in tests/test_gpu_blocktri_shapes.py: 1e-10 against an independent factorisation (np.linalg.inv of the Schur
blocks, scipy's sparse LU), 1e-12 in norm and elementwise against the two sweeps in long double on the blocks fetched from
the object (only the fp64 summation order differs).  The pivots themselves are not compared with the host: a near-tie may
be resolved differently after different rounding, and both results are valid inverses."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import blocktri_cases as bc
import blocktri_pivot_ref as pv
from conftest import rel_err

pytestmark = pytest.mark.gpu

NONE, PARTIAL, AUTO = 0, 1, 2
LSFC_EINVAL, LSFC_ENOMEM = -1, -3                       # include/lsfc.h
STORAGES = ("complex128", "complex64")
shapes = pytest.mark.parametrize("shape", pv.PERMUTED_SHAPES, ids=bc.shape_id)


def _both(x, ref):
    return rel_err(x, ref), bc.elementwise_err(x, ref)


def _lib():
    import fast_solver_lippmann_schwinger_amd._lib as L
    return L, L.load()


def _wrap(lsfc, pc, N):
    P = lsfc.SparsifyingPreconditioner.__new__(lsfc.SparsifyingPreconditioner)   # as from_operator wraps its handle
    P._pc, P.Msp, P.As, P.solverType, P.factor, P.N = pc, None, None, "UMFPACK", "blocktri", N
    return P


def _create(lsfc, Msp, As, K, pivoting=PARTIAL, prec=0, reserved=None, opts=True, entry="opts", N=None, arrays=True):
    """the C constructors on host arrays: (return code, object or None, message)"""
    L, lib = _lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    N = Msp.shape[0] if N is None else N
    if arrays:
        keep = (np.ascontiguousarray(Msp.indptr, dtype=np.int64), np.ascontiguousarray(Msp.indices, dtype=np.int64),
                np.ascontiguousarray(As.data, dtype=np.complex128), np.ascontiguousarray(Msp.data, dtype=np.complex128))
        ptrs = [p(a) for a in keep]
    else:
        ptrs = [C.c_void_p(8)] * 4                         # never read: the call must fail before it touches an array
    pc = C.c_void_p()
    if entry == "prec":
        rc = lib.lsfc_precond_create_blocktri_prec(C.byref(pc), N, K, *ptrs, L.LSFC_MEM_HOST, 0, prec)
    else:
        o = L.BlocktriOpts(inverse_precision=prec, pivoting=pivoting)
        for i, v in enumerate(reserved or ()):
            o.reserved[i] = v
        rc = lib.lsfc_precond_create_blocktri_opts(C.byref(pc), N, K, *ptrs, L.LSFC_MEM_HOST, 0, C.byref(o) if opts else None)
    msg = lib.lsfc_last_error().decode()
    if rc != 0 or not pc.value:
        return rc, None, msg
    return rc, _wrap(lsfc, pc, N), msg


def _blocks(P, K):
    return [P.blocktri_block(k) for k in range(K)]


def _is_permutation(perm, b):
    return perm.shape == (b,) and np.array_equal(np.sort(perm), np.arange(b))


# ---- 1. planted pivots ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [1e-9, 0.0])
def test_planted_pivots(lsfc, eps):
    b, K = pv.PLANT_B, pv.PLANT_K
    Msp, As = pv.planted(eps)
    rc, P, msg = _create(lsfc, Msp, As, K, pivoting=NONE)
    print(msg)
    assert rc != 0 and P is None
    assert "block 1 " in msg and "row 115 " in msg and "row 45 of the block" in msg and "needs pivoting" in msg, msg
    rc, P, msg = _create(lsfc, Msp, As, K, pivoting=PARTIAL)
    assert rc == 0 and P is not None, msg
    info = P.blocktri_info()
    assert info["pivoting"] == 1 and (info["blocks"], info["block_size"]) == (K, b)
    perm = P.blocktri_pivots(1)
    assert np.array_equal(np.nonzero(perm != np.arange(b))[0], [45, 46]) and perm[45] == 46 and perm[46] == 45, perm
    for k in (0, 2):
        assert _is_permutation(P.blocktri_pivots(k), b)
    S = bc.schur_blocks(Msp, K)
    got = _blocks(P, K)
    for k in range(K):
        err = _both(got[k], np.linalg.inv(S[k]))
        print(f"planted {eps:g}: block {k} vs np.linalg.inv {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
        assert err[0] <= 1e-10 and err[1] <= 1e-10
    v = bc.right_hand_sides(b * K, 1, seed=9)[0]
    w = As @ v
    x = P.solve(v)
    err = _both(x, spla.splu(Msp.tocsc()).solve(w))
    print(f"planted {eps:g}: apply vs splu {err[0]:.2e} / {err[1]:.2e}")
    assert err[0] <= 1e-10 and err[1] <= 1e-10
    err = _both(x, bc.solve_ld(Msp, got, w))
    print(f"planted {eps:g}: apply vs the long-double sweeps on the stored blocks {err[0]:.2e} / {err[1]:.2e}")
    assert err[0] <= 1e-12 and err[1] <= 1e-12
    got_ratio = info["min_pivot_ratio"]
    want_ratio = min(pv.gauss_jordan_partial(Sk)[2] for Sk in S)
    assert abs(got_ratio - want_ratio) <= 1e-10 * want_ratio
    P.close()


def test_planted_second(lsfc):
    """row 3 of block 2 holds a lone diagonal of 1e-12: the restatement decides on the host whether block 2 is singular
    under the rule, and the device must decide the same"""
    b, K = pv.PLANT_B, pv.PLANT_K
    Msp, As = pv.planted(1e-9, second=True)
    rc, P, msg = _create(lsfc, Msp, As, K, pivoting=NONE)
    assert rc != 0 and P is None and "block 1 " in msg and "row 45 of the block" in msg, msg
    S = bc.schur_blocks(Msp, K)
    ratios = [pv.gauss_jordan_partial(Sk)[2] for Sk in S]
    print(f"planted, second: smallest chosen |pivot| / max|S_k| per block on the host {ratios}")
    assert min(ratios[:2]) >= 1e-2 and not 1e-9 <= ratios[2] <= 1e-7          # block 2 is far from the threshold, either side
    rc, P, msg = _create(lsfc, Msp, As, K, pivoting=PARTIAL)
    print(msg)
    if ratios[2] < 1e-8:
        assert rc == LSFC_EINVAL and P is None
        assert "block 2 " in msg and "singular to working precision" in msg and "needs pivoting" not in msg, msg
    else:
        assert rc == 0 and P is not None, msg
        assert P.blocktri_info()["pivoting"] == 1
        err = _both(P.blocktri_block(2), np.linalg.inv(S[2]))
        assert err[0] <= 1e-10 and err[1] <= 1e-10
        P.close()


# ---- 2. permuted shapes -----------------------------------------------------------------------------------------------------

_OBJ = {}


def _objects(lsfc, shape):
    """{storage: PARTIAL object of the permuted pair}, its fetched blocks and pivots; built once per session, read only"""
    if shape not in _OBJ:
        b, K, _ = shape
        Mp, Ap = pv.case(shape)[:2]
        objs = {}
        for dt, prec in zip(STORAGES, (0, 1)):
            rc, P, msg = _create(lsfc, Mp, Ap, K, pivoting=PARTIAL, prec=prec)
            assert rc == 0 and P is not None, msg
            objs[dt] = (P, _blocks(P, K), [P.blocktri_pivots(k) for k in range(K)])
        _OBJ[shape] = objs
    return _OBJ[shape]


@shapes
def test_permuted_blocks(lsfc, shape):
    b, K, _ = shape
    Mp, Ap, perms, Msp, As = pv.case(shape)
    rc, P, msg = _create(lsfc, Mp, Ap, K, pivoting=NONE)
    if b > 2:                                              # (b = 2: tests/test_blocktri_pivot_cpu.py)
        assert rc != 0 and P is None and "needs pivoting" in msg, msg
    objs = _objects(lsfc, shape)
    P64, S64, piv64 = objs["complex128"]
    P32, S32, piv32 = objs["complex64"]
    S = bc.schur_blocks(Msp, K)
    worst = (0.0, 0.0)
    for k in range(K):
        want = np.linalg.inv(S[k])[:, perms[k]]            # (Pi_k S_k)^{-1} = S_k^{-1} Pi_k^T
        err = _both(S64[k], want)
        worst = max(worst[0], err[0]), max(worst[1], err[1])
        assert err[0] <= 1e-10 and err[1] <= 1e-10, f"block {k}: {err}"
        assert np.array_equal(S32[k], S64[k].astype(np.complex64).astype(np.complex128)), f"block {k}: not the fp64 block cast to float"
        assert _is_permutation(piv64[k], b) and np.array_equal(piv32[k], piv64[k])
    print(f"{bc.shape_id(shape)}: blocks vs np.linalg.inv {worst[0]:.2e} in norm, {worst[1]:.2e} elementwise")
    for P, per in ((P64, 16), (P32, 8)):
        info = P.blocktri_info()
        assert (info["blocks"], info["block_size"], info["factor_bytes"], info["pivoting"]) == (K, b, K * b * b * per, 1)
    want = min(pv.pivots_partial(Sk)[1] for Sk in bc.schur_blocks(Mp, K))
    got = P64.blocktri_info()["min_pivot_ratio"]
    print(f"{bc.shape_id(shape)}: min_pivot_ratio {got:.15e}, the restatement {want:.15e}")
    assert abs(got - want) <= 1e-10 * want
    assert P32.blocktri_info()["min_pivot_ratio"] == got


@shapes
def test_permuted_apply(lsfc, shape):
    b, K, _ = shape
    N = b * K
    Mp, Ap, perms, Msp, As = pv.case(shape)
    B = bc.right_hand_sides(N, 8)
    W = (Ap @ B.T).T
    rc, P0, msg = _create(lsfc, Msp, As, K, pivoting=NONE)  # the pair before the permutation, without pivoting
    assert rc == 0, msg
    plain = P0.solve(B[0])
    P0.close()
    for dt in STORAGES:
        P, blocks, _ = _objects(lsfc, shape)[dt]
        ref = bc.solve_ld(Mp, blocks, W)
        x = P.solve(B[0])
        err = _both(x, ref[0])
        print(f"{bc.shape_id(shape)} {dt}: apply vs the long-double sweeps on the stored blocks {err[0]:.2e} / {err[1]:.2e}")
        assert err[0] <= 1e-12 and err[1] <= 1e-12
        for R in (1, 5, 8):
            V = P.solve_batch(B[:R])
            for j in range(R):
                e = _both(V[j], ref[j])
                assert e[0] <= 1e-12 and e[1] <= 1e-12, f"{dt}: member {j} of {R}: {e}"
        if dt == "complex128":                             # Msp'^{-1} As' = Msp^{-1} As
            err = _both(x, plain)
            print(f"{bc.shape_id(shape)}: permuted pair with pivoting vs the pair itself without {err[0]:.2e} / {err[1]:.2e}")
            assert err[0] <= 1e-12 and err[1] <= 1e-12


@shapes
def test_permuted_repeatable(lsfc, shape):
    b, K, _ = shape
    Mp, Ap = pv.case(shape)[:2]
    for dt, prec in zip(STORAGES, (0, 1)):
        _, blocks, pivots = _objects(lsfc, shape)[dt]
        rc, P, msg = _create(lsfc, Mp, Ap, K, pivoting=PARTIAL, prec=prec)
        assert rc == 0, msg
        for k in range(K):
            assert np.array_equal(P.blocktri_block(k), blocks[k]), f"{dt}: block {k}"
            assert np.array_equal(P.blocktri_pivots(k), pivots[k]), f"{dt}: pivots of block {k}"
        P.close()


# ---- 3. tie rule, 4. singular under pivoting ------------------------------------------------------------------------------

def test_tie_rule(lsfc):
    Msp, As = pv.tie_pair()
    rc, P, msg = _create(lsfc, Msp, As, 1, pivoting=PARTIAL)
    assert rc == 0 and P is not None, msg
    perm = P.blocktri_pivots(0)
    assert _is_permutation(perm, 40) and perm[0] == 0, perm
    err = _both(P.blocktri_block(0), np.linalg.inv(Msp.toarray()))
    assert err[0] <= 1e-10 and err[1] <= 1e-10
    P.close()


def test_singular_under_pivoting(lsfc):
    Msp, As = pv.singular_pair()
    rc, P, msg = _create(lsfc, Msp, As, 2, pivoting=PARTIAL)
    print(msg)
    assert rc == LSFC_EINVAL and P is None
    assert "block 1 " in msg and "singular to working precision" in msg and "needs pivoting" not in msg, msg


# ---- 5. modes -----------------------------------------------------------------------------------------------------------------

def _same_object(P, Q, K, v):
    for k in range(K):
        assert np.array_equal(P.blocktri_block(k), Q.blocktri_block(k)), f"block {k}"
        assert np.array_equal(P.blocktri_pivots(k), Q.blocktri_pivots(k)), f"pivots of block {k}"
    assert np.array_equal(P.solve(v), Q.solve(v))
    B = np.stack([v, 2.0 * v, 1j * v])
    assert np.array_equal(P.solve_batch(B), Q.solve_batch(B))
    a, c = P.blocktri_info(), Q.blocktri_info()
    assert all(a[f] == c[f] for f in ("blocks", "block_size", "factor_bytes", "launches", "pivoting", "min_pivot_ratio"))


def _physical_2d(lsfc):
    from test_gpu_sparsify import case
    return tuple(lsfc.sparsifying_pair(case("trap", (33, 33, 1))[0])) + (33,)


@pytest.mark.parametrize("which", ["b129", "2d-n33"])
def test_mode_none_is_the_old_entry_point(lsfc, which):
    Msp, As, K = bc.built((129, 2, "scattered"))[:2] + (2,) if which == "b129" else _physical_2d(lsfc)
    v = bc.right_hand_sides(Msp.shape[0], 1, seed=21)[0]
    for prec in (0, 1):
        rc, old, msg = _create(lsfc, Msp, As, K, entry="prec", prec=prec)
        assert rc == 0, msg
        for kwargs in ({"pivoting": NONE, "prec": prec}, {"opts": False}) if prec == 0 else ({"pivoting": NONE, "prec": prec},):
            rc, new, msg = _create(lsfc, Msp, As, K, **kwargs)
            assert rc == 0, msg
            assert new.blocktri_info()["pivoting"] == 0
            assert np.array_equal(new.blocktri_pivots(K - 1), np.arange(Msp.shape[0] // K))
            _same_object(old, new, K, v)
            new.close()
        old.close()


def test_mode_auto(lsfc):
    # no breakdown: the NONE object
    Msp, As = bc.built((129, 2, "scattered"))[:2]
    v = bc.right_hand_sides(258, 1, seed=22)[0]
    rc, a, msg = _create(lsfc, Msp, As, 2, pivoting=AUTO)
    assert rc == 0, msg
    rc, n, msg = _create(lsfc, Msp, As, 2, pivoting=NONE)
    assert rc == 0, msg
    assert a.blocktri_info()["pivoting"] == 0
    _same_object(a, n, 2, v)
    a.close(), n.close()
    # breakdown: the PARTIAL object
    Msp, As = pv.planted(1e-9)
    v = bc.right_hand_sides(210, 1, seed=23)[0]
    rc, a, msg = _create(lsfc, Msp, As, 3, pivoting=AUTO)
    assert rc == 0, msg
    rc, p, msg = _create(lsfc, Msp, As, 3, pivoting=PARTIAL)
    assert rc == 0, msg
    assert a.blocktri_info()["pivoting"] == 1
    _same_object(a, p, 3, v)
    a.close(), p.close()


# ---- 6. argument checks, 7. memory rule -------------------------------------------------------------------------------------

def test_argument_checks(lsfc):
    L, lib = _lib()
    Msp, As = bc.built((16, 3, "scattered"))[:2]
    for kwargs, word in (({"pivoting": 3}, "pivoting"), ({"pivoting": -1}, "pivoting"), ({"prec": 2}, "inverse_precision"),
                         ({"reserved": (0, 0, 0, 0, 0, 1)}, "reserved"), ({"reserved": (7,)}, "reserved")):
        rc, P, msg = _create(lsfc, Msp, As, 3, **kwargs)
        assert rc == LSFC_EINVAL and P is None and word in msg, (kwargs, msg)
    rc, P, msg = _create(lsfc, Msp, As, 3, pivoting=PARTIAL)
    assert rc == 0, msg
    out = np.full(17, -7, dtype=np.int64)
    p = out.ctypes.data_as(C.c_void_p)
    assert lib.lsfc_precond_blocktri_get_pivots(P._pc, 0, p, 15) == LSFC_EINVAL and "capacity" in lib.lsfc_last_error().decode()
    assert lib.lsfc_precond_blocktri_get_pivots(P._pc, 3, p, 16) == LSFC_EINVAL
    assert lib.lsfc_precond_blocktri_get_pivots(P._pc, -1, p, 16) == LSFC_EINVAL
    assert lib.lsfc_precond_blocktri_get_pivots(P._pc, 0, None, 16) == LSFC_EINVAL
    assert np.all(out == -7)
    assert lib.lsfc_precond_blocktri_get_pivots(P._pc, 2, p, 16) == 0 and out[16] == -7 and _is_permutation(out[:16], 16)
    P.close()
    H = lsfc.SparsifyingPreconditioner(Msp, As)             # the host-LU route keeps no pivots of this kind
    assert lib.lsfc_precond_blocktri_get_pivots(H._pc, 0, p, 16) == LSFC_EINVAL
    H.close()
    with pytest.raises(ValueError):
        lsfc.SparsifyingPreconditioner(Msp, As, pivoting="partial")
    with pytest.raises(ValueError):
        lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=3, pivoting="full")
    Q = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=3, pivoting="auto")
    assert Q.blocktri_info()["pivoting"] == 0 and np.array_equal(Q.blocktri_pivots(1), np.arange(16))
    Q.close()


def test_memory_rule(lsfc):
    """256^3 (b = 65 536, 256 blocks: 17.6 TB of inverses) must fail from the dimensions alone, under PARTIAL and AUTO too"""
    for mode in (PARTIAL, AUTO):
        rc, P, msg = _create(lsfc, None, None, 256, pivoting=mode, N=256 ** 3, arrays=False)
        assert rc == LSFC_ENOMEM and P is None and "GB" in msg, msg


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,dims", [("trap", (33, 33, 1)), ("gv3", (12, 12, 12))])
def test_gmres_with_pivoting(lsfc, kind, dims):
    from oracle import lsfc_oracle as o
    from test_gpu_sparsify import case
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
    Pn = lsfc.SparsifyingPreconditioner.from_operator(M)
    Pp = lsfc.SparsifyingPreconditioner.from_operator(M, pivoting="partial")
    assert Pn.blocktri_info()["pivoting"] == 0 and Pp.blocktri_info()["pivoting"] == 1
    b = Pp.blocktri_info()["block_size"]
    assert _is_permutation(Pp.blocktri_pivots(0), b)
    un, hn = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=Pn, reltol=1e-6, log=True)
    up, hp = lsfc.gmres_(np.zeros(N, dtype=np.complex128), M, rhs, Pl=Pp, reltol=1e-6, log=True)
    print(f"{kind} {dims}: {hp.iters} iterations with partial pivoting, {hn.iters} without; solutions differ by {rel_err(up, un):.2e}; "
          f"min pivot ratio {Pp.blocktri_info()['min_pivot_ratio']:.3f} against {Pn.blocktri_info()['min_pivot_ratio']:.3f}")
    assert hn.isconverged and hp.isconverged and hp.iters == hn.iters
    assert rel_err(up, un) <= 1e-10
