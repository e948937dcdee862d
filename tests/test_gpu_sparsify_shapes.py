"""GPU tests of the sparsifying assembly (csrc/sparsify.hip, lsfc_sparsify_build) on the grids of tests/sparsify_cases.py:
several tiles per workgroup in k_gram / k_refine, rectangles in both orientations, the smallest grids, ill-conditioned
classes; and the state around the call (op, nu, NULL arrays, memspace), the refusals, and the evenness requirement of the
kernel.  Reference: the restatement of tests/sparsify_ref.py, computed once per case (sparsify_cases.reference).

Bound per class c, for As, AG and Msp after per-row phase alignment: relative l2 error <= min(1e-9, tol_c),

    tol_c = (MARGIN eps + 2 delta_c) sigma_max / (sigma_-2 - sigma_min)

eps sigma_max / (sigma_-2 - sigma_min) = b_c is the accuracy of the SVD reference's vector; MARGIN = 4 x the largest ratio
e / b_c of the device algorithm emulated in numpy double (sparsify_cases.MARGIN: measured on the CPU, never on the device).
delta_c is measured here: the relative l2 difference between the device's and the restatement's row of G for the first
sample source of class c (the other rows of a class are the same kernel one grid point further).  The two sides evaluate G by
different FFTs and Bessel routines, and a relative perturbation delta of the rows moves the vector by delta sigma_max /
(sigma_-2 - sigma_min): that is not an error of the assembly.  delta_c <= 1e-12 is asserted on its own (the apply's tests sit
near 1e-15), so a wrong kernel cannot widen its own tolerance.  sigma: |sigma_dev - sigma_ref| <= (MARGIN eps + 2 delta_c)
sigma_max in all three columns.  The figures every case prints are in DESIGN.md, "Sparsifying matrices"."""
import ctypes as C

import numpy as np
import pytest

import sparsify_cases as sc
import sparsify_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
NAMES = ("rowptr", "col", "As", "AG", "Msp", "sigma")


def _lib():
    import fast_solver_lippmann_schwinger_amd._lib as L
    return L, L.load()


def _csr(A):
    A = A.tocsr()
    A.sort_indices()
    return A


def _row_phase(dev, rf, rowptr):
    """per-row unit factor p with dev * p ~ rf (the singular vector of a class is defined up to one)"""
    N = rowptr.size - 1
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    z = np.conj(dev) * rf
    s = np.bincount(rows, weights=z.real, minlength=N) + 1j * np.bincount(rows, weights=z.imag, minlength=N)
    return (s / np.abs(s))[rows]


def _build_raw(M, want=NAMES):
    """lsfc_sparsify_build into host arrays for the names in `want` only, NULL for the others; (rc, arrays)"""
    L, lib = _lib()
    n, m, l = _dims(M)
    N = n * m * l
    nnz = C.c_int64(0)
    L.check(lib.lsfc_sparsify_pattern(n, m, l, C.byref(nnz), None, None, None))
    shape = dict(rowptr=(N + 1, np.int64), col=(nnz.value, np.int64), As=(nnz.value, np.complex128), AG=(nnz.value, np.complex128),
                 Msp=(nnz.value, np.complex128), sigma=((9 if l == 1 else 27, 3), np.float64))
    out = {k: (np.full(shape[k][0], -7, dtype=shape[k][1]) if k in want else None) for k in NAMES}
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib.lsfc_sparsify_build(M._plan, *(p(out[k]) for k in NAMES), L.LSFC_MEM_HOST)
    return rc, out


def _dims(M):
    L, lib = _lib()
    d = (C.c_int64 * 3)()
    L.check(lib.lsfc_plan_dims(M._plan, d, None))
    return int(d[0]), int(d[1]), int(d[2])


def _sample(M, sources):
    """(rc, rows) of lsfc_sample_sources"""
    L, lib = _lib()
    src = np.ascontiguousarray(sources, dtype=np.int64)
    out = np.empty((src.size, M.N), dtype=np.complex128)
    rc = lib.lsfc_sample_sources(M._plan, src.ctypes.data_as(C.c_void_p), src.size, out.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST)
    return rc, out


def _delta_rows(M, r):
    """delta_c of the module docstring, one per class"""
    first = [int(np.asarray(sA)[0]) - 1 for sA, _, _, _ in r["classes"]]
    rc, rows = _sample(M, first)
    assert rc == 0
    return np.array([rel_err(rows[c], r["row0"][c]) for c in range(len(first))])


def _judge(d, r, delta, names, what, Msp_ref=None):
    """pattern, values per class, sigma and the phase convention of the device arrays d against the restatement r.
    Prints the largest error of each array in units of b_c, and delta, before it asserts."""
    mats = {"As": _csr(r["As"]), "AG": _csr(r["AG"])}
    if "Msp" in names:
        mats["Msp"] = _csr(r["Msp"] if Msp_ref is None else Msp_ref)
    As = mats["As"]
    assert np.array_equal(d["rowptr"], As.indptr) and np.array_equal(d["col"], As.indices)
    N = As.shape[0]
    s = r["sigma"]
    nclass = s.shape[0]
    amp = s[:, 0] / (s[:, 1] - s[:, 2])                     # sigma_max / (sigma_-2 - sigma_min)
    b = sc.EPS * amp
    tol = np.minimum(1e-9, (sc.MARGIN * sc.EPS + 2.0 * delta) * amp)
    ph = _row_phase(d["As"], As.data, d["rowptr"])
    cls = r["row_class"][np.repeat(np.arange(N), np.diff(d["rowptr"]))]
    err = {name: np.array([rel_err(d[name][cls == c] * ph[cls == c], mats[name].data[cls == c]) for c in range(nclass)]) for name in names}
    dsig = np.abs(d["sigma"] - s) / s[:, :1]
    print(f"{what}: " + ", ".join(f"{name} <= {(err[name] / b).max():.2f} b_c" for name in names)
          + f", delta_rows <= {delta.max():.1e}, |dsigma|/sigma_max <= {dsig.max():.1e}, smallest tol_c {tol.min():.1e}, largest {tol.max():.1e}")
    assert np.all(delta <= 1e-12), delta
    # (class, error, tol_c, error / b_c) of everything over the bound, all arrays in one report
    over = {name: [(int(c), float(err[name][c]), float(tol[c]), float(err[name][c] / b[c])) for c in np.flatnonzero(~(err[name] <= tol))]
            for name in names}
    assert not any(over.values()), (what, {k: v for k, v in over.items() if v})
    assert np.all(dsig <= (sc.MARGIN * sc.EPS + 2.0 * delta)[:, None]), (what, dsig / sc.EPS)
    # the phase convention: the largest entry of each stencil is real and positive
    for c in range(nclass):
        row = int(np.flatnonzero(r["row_class"] == c)[0])
        v = d["As"][d["rowptr"][row]:d["rowptr"][row + 1]]
        top = v[np.argmax(np.abs(v))]
        assert top.imag == 0.0 and top.real > 0, (c, top)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_device_build_matches_restatement(lsfc, case):
    r = sc.reference(case)
    M = sc.device_operator(lsfc, case)
    names = ("As", "AG") if case.kind == "lowk" else ("As", "AG", "Msp")
    d = lsfc.sparsify_arrays(M, names)
    _judge(d, r, _delta_rows(M, r), names, f"{sc.case_id(case)} {sc.tiles(case)}")
    if case.kind == "lowk":                                # the entries a user calls return what the raw call returned
        g = sc.geometry(case)
        args = (g.k, g.coords[0], g.coords[1], g.D0, *case.dims)
        assert np.array_equal(_csr(lsfc.buildSparseA(*args)).data, d["As"])
        assert np.array_equal(_csr(lsfc.buildSparseAG(*args)).data, d["AG"])


BITWISE = [sc.find("trap", (129, 129)), sc.find("gv3", (26, 26, 26))]


@pytest.mark.parametrize("case", BITWISE, ids=sc.case_id)
def test_repeat_and_device_memspace_are_bitwise_equal(lsfc, case):
    # the fixed summation order, with partials that hold two tiles
    import torch
    L, lib = _lib()
    M = sc.device_operator(lsfc, case)
    a, b = lsfc.sparsify_arrays(M), lsfc.sparsify_arrays(M)
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name
    N, nnz = a["rowptr"].size - 1, a["col"].size
    nclass = a["sigma"].shape[0]
    t = dict(rowptr=torch.empty(N + 1, dtype=torch.int64, device="cuda"), col=torch.empty(nnz, dtype=torch.int64, device="cuda"),
             As=torch.empty(nnz, dtype=torch.complex128, device="cuda"), AG=torch.empty(nnz, dtype=torch.complex128, device="cuda"),
             Msp=torch.empty(nnz, dtype=torch.complex128, device="cuda"), sigma=torch.empty((nclass, 3), dtype=torch.float64, device="cuda"))
    L.check(lib.lsfc_sparsify_build(M._plan, *(C.c_void_p(t[k].data_ptr()) for k in NAMES), L.LSFC_MEM_DEVICE))
    torch.cuda.synchronize()
    for name in NAMES:
        assert np.array_equal(t[name].cpu().numpy(), a[name]), name


def test_null_arrays_leave_the_others_unchanged(lsfc):
    M = sc.device_operator(lsfc, sc.find("gv3", (26, 26, 26)))
    rc, full = _build_raw(M)
    assert rc == 0
    for want in (("Msp",), ("rowptr", "col"), ("sigma",)):
        rc, part = _build_raw(M, want)
        assert rc == 0, want
        for name in NAMES:
            if name in want:
                assert np.array_equal(part[name], full[name]), (want, name)
            else:
                assert part[name] is None


@pytest.mark.parametrize("case", [sc.find("gv3", (4, 6, 8)), sc.find("trap", (129, 129))], ids=sc.case_id)
def test_the_op_of_the_plan_is_not_read(lsfc, case):
    L, lib = _lib()
    M = sc.device_operator(lsfc, case)
    rc, base = _build_raw(M)
    assert rc == 0
    try:
        for op in (L.LSFC_OP_T, L.LSFC_OP_H):
            L.check(lib.lsfc_plan_set_op(M._plan, op))
            rc, got = _build_raw(M)
            assert rc == 0
            for name in NAMES:
                assert np.array_equal(got[name], base[name]), (op, name)
            now = C.c_int(-7)
            L.check(lib.lsfc_plan_get_op(M._plan, C.byref(now)))
            assert now.value == op
    finally:
        L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N))


@pytest.mark.parametrize("case", [sc.find("trap", (21, 41)), sc.find("gv3", (4, 6, 8))], ids=sc.case_id)
def test_nu_is_read_again_and_the_kernel_is_kept(lsfc, case):
    r = sc.reference(case)
    M = sc.device_operator(lsfc, case)
    rc, first = _build_raw(M)
    assert rc == 0
    nu_new = sc.nu_of(case, other=True)
    assert rel_err(nu_new, sc.nu_of(case)) > 0.5
    M.set_nu(nu_new)
    rc, second = _build_raw(M)
    assert rc == 0
    for name in ("rowptr", "col", "As", "AG", "sigma"):
        assert np.array_equal(second[name], first[name]), name
    assert not np.array_equal(second["Msp"], first["Msp"])
    import scipy.sparse as sp
    Msp_ref = (r["As"] + sc.geometry(case).k ** 2 * (r["AG"] @ sp.diags(nu_new))).tocsc()
    _judge(second, r, _delta_rows(M, r), ("As", "AG", "Msp"), f"{sc.case_id(case)} after set_nu", Msp_ref=Msp_ref)


def test_grids_too_small_are_refused(lsfc):
    L, lib = _lib()
    # 3D: 3 x 4 x 4 = 48 points, fewer than twice the 27 sources of the interior stencil (a literal plan: the builder takes
    # even axes only)
    n, m, l = 3, 4, 4
    G = np.ones((2 * n, 2 * m, 2 * l), dtype=np.complex128)     # a constant symbol: the kernel is a unit source, even in every axis
    M3 = lsfc.FastM3D(G, np.zeros(n * m * l), 2 * n, 2 * m, 2 * l, n, m, l, 2.0)
    # 2D: 3 x 3 = 9 points against the 9 sources of the interior stencil
    h = 0.5
    x = h * (np.arange(3) - 1.0)
    M2 = lsfc.buildFastConvolution(x, x, h, 1.0 / h, sc.nu2, quadRule="trapezoidal")
    for M in (M3, M2):
        rc, out = _build_raw(M)
        assert rc == L.LSFC_EINVAL
        msg = lib.lsfc_last_error().decode()
        assert "sparsify" in msg and "too small" in msg, msg
        assert np.all(out["sigma"] == -7) and np.all(out["col"] == -7)      # nothing was written


# ---- the kernel has to be even in every axis: the gathers read K[|i - s|] -------------------------------------------------
LITERAL = sorted(sc.LITERAL)
_lid = lambda d: "x".join(map(str, d))   # noqa: E731


def _refused(rc, entry):
    L, lib = _lib()
    assert rc == L.LSFC_EINVAL, (entry, rc)
    msg = lib.lsfc_last_error().decode()
    assert "not even along axis" in msg and "deviation" in msg and entry in msg, msg
    return msg


@pytest.mark.parametrize("symmetry", ["none", "point"])
@pytest.mark.parametrize("dims", LITERAL, ids=_lid)
def test_a_kernel_that_is_not_even_is_refused(lsfc, dims, symmetry):
    L, lib = _lib()
    M = sc.literal_operator(lsfc, dims, symmetry)
    if symmetry == "point":
        # symmetric as a matrix: the op code's check passes, and must not be what decides here
        assert M.symmetry_defect() <= 1e-10
        L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_T))
        L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N))
    else:
        assert M.symmetry_defect() > 1e-3
    rc, rows = _sample(M, [0, M.N // 2])
    print(_refused(rc, "lsfc_sample_sources"))
    rc, out = _build_raw(M)
    _refused(rc, "sparsify")
    assert np.all(out["sigma"] == -7) and np.all(out["As"] == -7)
    pc = C.c_void_p()
    rc = lib.lsfc_precond_create_from_plan(C.byref(pc), M._plan)
    _refused(rc, "sparsify")
    assert not pc.value
    # the apply itself is not concerned
    b = np.random.default_rng(1).standard_normal(M.N) + 0j
    from oracle import lsfc_oracle as o
    want = o.apply_reduced(sc.literal_symbol(dims, symmetry), sc.literal_nu(dims), sc.LITERAL_OMEGA, b, dims)
    assert rel_err(M * b, want) <= 1e-10


def test_trapezoidal_grid_off_centre(lsfc):
    # the trapezoidal builder's kernel is the distance to the centre of the extended grid (src/FastConvolution.jl:433-434): on a
    # grid that is not centred at the origin it is not even, and the plan is measured instead of trusted
    from oracle import lsfc_oracle as o
    n = 21
    h = 1.0 / (n - 1)
    x = np.linspace(0.0, 1.0, n)
    M = lsfc.buildFastConvolution(x, x, h, 1.0 / h, sc.nu2, quadRule="trapezoidal")
    rc, _ = _sample(M, [0])
    _refused(rc, "lsfc_sample_sources")
    rc, _ = _build_raw(M)
    _refused(rc, "sparsify")
    # buildSparseA / buildSparseAG read distances only (sampleG): the grid's position does not matter to them
    X, Y = o.grid2d(x, x)
    D0 = o.reference_vals_trap_rule()[1][0]
    k = 1.0 / h
    r = ref.build(ref.direct_rows(k, X, Y, D0, h), n, n)
    As, AG = _csr(lsfc.buildSparseA(k, X, Y, D0, n, n)), _csr(lsfc.buildSparseAG(k, X, Y, D0, n, n))
    ph = _row_phase(As.data, _csr(r["As"]).data, As.indptr)
    assert rel_err(As.data * ph, _csr(r["As"]).data) <= 1e-9 and rel_err(AG.data * ph, _csr(r["AG"]).data) <= 1e-9


@pytest.mark.parametrize("dims", LITERAL, ids=_lid)
def test_an_even_literal_kernel_is_sampled_and_assembled(lsfc, dims):
    """(The symbols carry a self term, sparsify_cases.SELF: without it a_c G[S_c, S_c] of the 3D case cancels 102-fold, and
    the AG rows of the device and of the numpy emulation alike are 6.5 ... 15.5 b_c from the SVD's with the vector within
    0.67 b_c of it -- the reference cannot judge an AG row at tol_c there.)"""
    r = sc.literal_reference(dims)
    M = sc.literal_operator(lsfc, dims, "axes")
    N = M.N
    sources = [0, N - 1, N // 2, N // 3, dims[0] - 1, N - dims[0]]
    rc, rows = _sample(M, sources)
    assert rc == 0
    want = ref.literal_rows(sc.literal_symbol(dims, "axes"), dims)(sources)
    for i, s in enumerate(sources):
        assert rel_err(rows[i], want[i]) <= 1e-12, (s, rel_err(rows[i], want[i]))
    d = lsfc.sparsify_arrays(M)
    _judge(d, r, _delta_rows(M, r), ("As", "AG", "Msp"), f"literal {dims}, symmetrised axis by axis")
