"""Assembly of the sparsifying preconditioner's matrices on the device (csrc/sparsify.hip, lsfc_sparsify_build):

    As  = buildSparseA(k, X, Y, D0, n, m)                    src/SparsifyingMatrix2D.jl:806-884
    AG  = buildSparseAG(k, X, Y, D0, n, m)                   src/SparsifyingMatrix2D.jl:351-438
    buildSparseAConv / buildSparseAGConv(k, X, Y, fastconv, n, m)              :888-966, :441-532
    buildSparseA3DConv / buildSparseAG3DConv(k, X, Y, Z, fastconv, n, m, l)    src/SparsifyingMatrix3D.jl:1410-1918
    Msp = As + k^2 AG diag(nu)                               examples/example.jl:67, examples/example3D.jl:61

The matrices come back as scipy.sparse CSC matrices, as the reference returns SparseMatrixCSC.  `sparsifying_pair`
returns (Msp, As) of one device call, ready for SparsifyingPreconditioner(Msp, As).  The singular-vector phase is
fixed (include/lsfc.h): the entry of largest modulus of every stencil is real and positive."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def nclasses(ndim):
    return 9 if ndim == 2 else 27


def sparsify_pattern(n, m, l=1):
    """(rowptr, col, row_class) of the common pattern of As / AG / Msp (lsfc_sparsify_pattern, host arithmetic)."""
    lib = L.load()
    nnz = C.c_int64(0)
    L.check(lib.lsfc_sparsify_pattern(int(n), int(m), int(l), C.byref(nnz), None, None, None))
    N = int(n) * int(m) * int(l)
    rowptr = np.empty(N + 1, dtype=np.int64)
    col = np.empty(nnz.value, dtype=np.int64)
    cls = np.empty(N, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    L.check(lib.lsfc_sparsify_pattern(int(n), int(m), int(l), C.byref(nnz), p(rowptr), p(col), p(cls)))
    return rowptr, col, cls


def _dims(M):
    d = (C.c_int64 * 3)()
    L.check(L.load().lsfc_plan_dims(M._plan, d, None))
    return int(d[0]), int(d[1]), int(d[2])


def sparsify_arrays(M, values=("As", "AG", "Msp")):
    """One lsfc_sparsify_build on the plan of `M` (FastM / FastM3D), host arrays:
    dict with rowptr, col, the requested value arrays (complex128) and sigma[nclass, 3] (max, second smallest, min)."""
    n, m, l = _dims(M)
    ndim = 2 if l == 1 else 3
    lib = L.load()
    nnz = C.c_int64(0)
    L.check(lib.lsfc_sparsify_pattern(n, m, l, C.byref(nnz), None, None, None))
    N = n * m * l
    out = {"rowptr": np.empty(N + 1, dtype=np.int64), "col": np.empty(nnz.value, dtype=np.int64),
           "sigma": np.empty((nclasses(ndim), 3), dtype=np.float64)}
    for v in ("As", "AG", "Msp"):
        out[v] = np.empty(nnz.value, dtype=np.complex128) if v in values else None
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    L.check(lib.lsfc_sparsify_build(M._plan, p(out["rowptr"]), p(out["col"]), p(out["As"]), p(out["AG"]), p(out["Msp"]),
                                    p(out["sigma"]), L.LSFC_MEM_HOST))
    return out


def _csc(arrs, name):
    import scipy.sparse as sp
    N = arrs["rowptr"].size - 1
    return sp.csr_matrix((arrs[name], arrs["col"], arrs["rowptr"]), shape=(N, N)).tocsc()


def _check(k, M, dims):
    if float(k) != float(M.omega):
        raise ValueError(f"k = {k!r} differs from the k of the fast convolution ({M.omega!r}): the rows of G are the plan's")
    if tuple(int(v) for v in dims) != _dims(M)[:len(dims)] or (len(dims) == 2 and _dims(M)[2] != 1):
        raise ValueError(f"DimensionMismatch: grid {tuple(dims)} but the fast convolution is {_dims(M)}")


def _direct_plan(k, X, Y, D0, n, m):
    """trapezoidal plan of the grid with nu = 0: its kernel is sampleG's (src/FastConvolution.jl:497-513 with D0).
    sampleG reads distances between grid points only, so the plan is made for the same grid centred at the origin: the
    builder's kernel is the distance to the centre of the extended grid, which is sampleG's only there."""
    from .operators import FastM
    X = np.asarray(X, float)
    n, m = int(n), int(m)
    h = abs(X[1] - X[0])
    D0 = complex(D0)
    nu = np.zeros(n * m)
    plan = C.c_void_p()
    L.check(L.load().lsfc_plan_create_trap2d(C.byref(plan), n, m, -(n - 1) / 2.0 * h, -(m - 1) / 2.0 * h, float(h), float(k),
                                             D0.real, D0.imag, nu.ctypes.data_as(C.c_void_p), 0, 0))
    return FastM(None, nu, 2 * n - 1, 2 * m - 1, n, m, k, quadRule="trapezoidal", _plan=plan)


def buildSparseA(k, X, Y, D0, n, m, method="normal"):
    """src/SparsifyingMatrix2D.jl:806-884 (rows of sampleG with the caller's D0)."""
    _method(method)
    return _csc(sparsify_arrays(_direct_plan(k, X, Y, D0, n, m), ("As",)), "As")


def buildSparseAG(k, X, Y, D0, n, m, method="normal"):
    """src/SparsifyingMatrix2D.jl:351-438."""
    _method(method)
    return _csc(sparsify_arrays(_direct_plan(k, X, Y, D0, n, m), ("AG",)), "AG")


def buildSparseAConv(k, X, Y, fastconv, n, m, method="normal"):
    """src/SparsifyingMatrix2D.jl:888-966."""
    _method(method)
    _check(k, fastconv, (n, m))
    return _csc(sparsify_arrays(fastconv, ("As",)), "As")


def buildSparseAGConv(k, X, Y, fastconv, n, m, method="normal"):
    """src/SparsifyingMatrix2D.jl:441-532."""
    _method(method)
    _check(k, fastconv, (n, m))
    return _csc(sparsify_arrays(fastconv, ("AG",)), "AG")


def buildSparseA3DConv(k, X, Y, Z, fastconv, n, m, l, method="normal"):
    """src/SparsifyingMatrix3D.jl:1410-1654."""
    _method(method)
    _check(k, fastconv, (n, m, l))
    return _csc(sparsify_arrays(fastconv, ("As",)), "As")


def buildSparseAG3DConv(k, X, Y, Z, fastconv, n, m, l, method="normal"):
    """src/SparsifyingMatrix3D.jl:1659-1913 (the definition that Julia keeps: it overrides the one at :705)."""
    _method(method)
    _check(k, fastconv, (n, m, l))
    return _csc(sparsify_arrays(fastconv, ("AG",)), "AG")


def sparsifying_pair(fastconv):
    """(Msp, As) with Msp = As + k^2 AG diag(nu) (nu, k of the plan), from one device call."""
    a = sparsify_arrays(fastconv, ("As", "Msp"))
    return _csc(a, "Msp"), _csc(a, "As")


def _method(method):
    if method != "normal":
        # the reference's "randomized" branch calls entriesSparseARand, which it never defines
        raise NameError(f"UndefVarError: entriesSparseARand not defined (method {method!r})")
