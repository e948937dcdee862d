"""numpy/scipy restatement of the reference's sparsifying-matrix assembly (test infrastructure, not product code).

    entriesSparseA / entriesSparseAConv      src/SparsifyingMatrix2D.jl:5-102, :104-201
    entriesSparseG / entriesSparseGConv      src/SparsifyingMatrix2D.jl:205-275, :278-350
    buildSparseAG(Conv) / buildSparseA(Conv) src/SparsifyingMatrix2D.jl:351-532, :806-966
    entriesSparseA3D                         src/SparsifyingMatrix3D.jl:1136-1406
    entriesSparseG3D                         src/SparsifyingMatrix3D.jl:963-1131
    buildSparseA3DConv / buildSparseAG3DConv src/SparsifyingMatrix3D.jl:1410-1654, :1659-1913
    createIndices                            src/Functions.jl:7-29

Every stencil, sample point and row set is written as the reference writes it (1-based, column-major, converted
with `- 1` at the end).  `rows(idx)` returns G[idx, :] (len(idx) x N) of the kernel under test: see direct_rows,
conv_rows and gv3d_rows.  SVDs are np.linalg.svd of the explicit rows; assembly is COO -> CSC."""
import numpy as np
import scipy.sparse as sp
import scipy.special as ss

from oracle import lsfc_oracle as o


# ---- rows of G --------------------------------------------------------------------------------------------------
def direct_rows(k, X, Y, D0, h):
    """sampleG: rows of the build_conv_matrix formula (src/FastConvolution.jl:497-513), one row at a time."""
    X, Y = np.asarray(X, float), np.asarray(Y, float)

    def rows(idx):
        out = np.empty((len(idx), X.size), dtype=np.complex128)
        for i, ii in enumerate(idx):
            r = np.sqrt((X - X[ii]) ** 2 + (Y - Y[ii]) ** 2)
            r[ii] = 1.0
            out[i] = 1j / 4 * ss.hankel1(0, k * r) * h ** 2
            out[i, ii] = 1j / 4 * D0 * h ** 2
        return out
    return rows


def conv_rows(fastconv):
    """sampleGConv through the oracle's FFTconvolution (2D Greengard-Vico oracle FastM)."""
    return lambda idx: o.sample_g_conv(list(idx), fastconv)


def gv3d_rows(n, m, l, box, k):
    """sampleG3D of the 3D Greengard-Vico plan: reduced_symbol_gv3d + convolve_reduced on unit sources (covers odd and
    non-cube shapes, as lsfc_plan_create_gv3d does)."""
    return literal_rows(o.reduced_symbol_gv3d(n, m, l, box, k), (n, m, l))


def literal_rows(G2, dims):
    """rows of an arbitrary reduced symbol G2 (plain FFT order, at least 2 n points per axis) on the grid `dims` (2D or
    3D): o.convolve_reduced on unit sources, one FFT convolution per row.  Nothing here assumes a symmetry of G2."""
    dims = tuple(int(v) for v in dims)
    N = int(np.prod(dims))

    def rows(idx):
        out = np.empty((len(idx), N), dtype=np.complex128)
        for i, ii in enumerate(idx):
            e = np.zeros(N, dtype=np.complex128)
            e[ii] = 1.0
            out[i] = o.convolve_reduced(G2, e, dims)
        return out
    return rows


# ---- the device algorithm, restated ---------------------------------------------------------------------------------
def gram_refine(Gs):
    """csrc/sparsify.hip in numpy double, for one class: H = Gs Gs^H, its eigenpairs (eigh in place of the cyclic Jacobi),
    the smallest pair (lam, u); from the rows themselves w = Gs (Gs^H u) and lam' = |Gs^H u|^2; one first-order correction
    of u against the other eigenvectors, u + sum_b v_b (v_b^H w) / (lam' - lam_b).  Returns (corrected, uncorrected), both
    of unit norm: approximations of the left singular vector of Gs for its smallest singular value."""
    H = Gs @ Gs.conj().T
    lam, V = np.linalg.eigh(H)
    u0 = V[:, 0]
    y = Gs.conj().T @ u0
    w = Gs @ y
    lmin = np.vdot(y, y).real
    u = u0.copy()
    for b in range(1, len(lam)):
        den = lmin - lam[b]
        if den != 0.0:
            u = u + V[:, b] * (np.vdot(V[:, b], w) / den)
    return u / np.linalg.norm(u), u0


def phase_distance(v, u):
    """2-norm distance of the unit vectors v and u after the unit factor that brings v closest to u"""
    s = np.vdot(v, u)
    return float(np.linalg.norm(v * (s / abs(s)) - u))


# ---- class tables -------------------------------------------------------------------------------------------------
def _F(a):
    return np.asarray(a).reshape(-1, order="F")


def classes_2d(n, m):
    """[(sample sources A (1-based), Indices, sample sources G (1-based), rows (1-based))] of the 9 classes."""
    assert n % 2 == 1
    IR = np.array([[-n - 1, -n, -n + 1], [-1, 0, 1], [n - 1, n, n + 1]])
    N = n * m
    Ind = np.arange(1, N + 1).reshape((n, m), order="F")
    c = n * (m - 1) // 2
    cls = []
    # (entriesSparseA sample, Indices) | entriesSparseG sample | buildSparseA rows
    cls.append((c + (n + 1) // 2 + _F(IR), _F(IR), c + (n + 1) // 2 + _F(IR), _F(Ind[1:-1, 1:-1])))
    cls.append((c + 1 + _F(IR[:, 1:3]), _F(IR[:, 1:3]), c + 1 + np.array([0, 1, n, n + 1, -n, -n + 1]), _F(Ind[0, 1:-1])))
    cls.append((c + _F(IR[:, 0:2]), _F(IR[:, 0:2]), c + np.array([-1, 0, n, n - 1, -n, -n - 1]), _F(Ind[-1, 1:-1])))
    cls.append(((n + 1) // 2 + _F(IR[1:3, :]), _F(IR[1:3, :]), (n + 1) // 2 + np.array([-1, 0, 1, n, n + 1, n - 1]),
                _F(Ind[1:-1, 0])))
    cls.append((N - (n + 1) // 2 + _F(IR[0:2, :]), _F(IR[0:2, :]), N - (n + 1) // 2 + np.array([-1, 0, 1, -n, -n + 1, -n - 1]),
                _F(Ind[1:-1, -1])))
    cls.append((1 + _F(IR[1:3, 1:3]), _F(IR[1:3, 1:3]), 1 + np.array([0, 1, n, n + 1]), np.array([Ind[0, 0]])))
    cls.append((n + _F(IR[1:3, 0:2]), _F(IR[1:3, 0:2]), n + np.array([0, -1, n, n - 1]), np.array([Ind[-1, 0]])))
    cls.append((n * m - n + 1 + np.array([0, 1, -n, -n + 1]), np.array([0, 1, -n, -n + 1]),
                n * m - n + 1 + np.array([0, 1, -n, -n + 1]), np.array([Ind[0, -1]])))
    cls.append((n * m + np.array([0, -1, -n, -n - 1]), np.array([0, -1, -n, -n - 1]),
                n * m + np.array([0, -1, -n, -n - 1]), np.array([Ind[-1, -1]])))
    return cls


def _julia_half(n):
    """round(Integer, n/2): ties to even (Python's round does the same)"""
    return int(round(n / 2))


def classes_3d(n, m, l):
    IR = np.zeros((3, 3, 3), dtype=np.int64)
    IR[:, :, 0] = np.array([[-m * n - n - 1, -m * n - n, -m * n - n + 1],
                            [-m * n - 1, -m * n, -m * n + 1],
                            [-m * n + n - 1, -m * n + n, -m * n + n + 1]]).T
    IR[:, :, 1] = np.array([[-n - 1, -n, -n + 1], [-1, 0, 1], [n - 1, n, n + 1]]).T
    IR[:, :, 2] = np.array([[m * n - n - 1, m * n - n, m * n - n + 1],
                            [m * n - 1, m * n, m * n + 1],
                            [m * n + n - 1, m * n + n, m * n + n + 1]]).T
    nH, mH, lH = _julia_half(n), _julia_half(m), _julia_half(l)
    ci = lambda i, j, kk: (kk - 1) * n * m + (j - 1) * n + i                          # changeInd3D  # noqa: E731

    def sub(i, j, kk):                                                              # subStencil3D
        return _F(IR[max(i - 1, 1) - 1:min(i + 1, 3), max(j - 1, 1) - 1:min(j + 1, 3), max(kk - 1, 1) - 1:min(kk + 1, 3)])
    Ind = np.arange(1, n * m * l + 1).reshape((n, m, l), order="F")
    I_ = slice(1, -1)
    spec = [  # (sample point, stencil, rows of buildSparseA3DConv)
        ((nH, mH, lH), _F(IR), Ind[I_, I_, I_]),
        ((1, mH, lH), _F(IR[1:3, :, :]), Ind[0, I_, I_]), ((n, mH, lH), _F(IR[0:2, :, :]), Ind[-1, I_, I_]),
        ((nH, 1, lH), _F(IR[:, 1:3, :]), Ind[I_, 0, I_]), ((nH, m, lH), _F(IR[:, 0:2, :]), Ind[I_, -1, I_]),
        ((nH, mH, 1), _F(IR[:, :, 1:3]), Ind[I_, I_, 0]), ((nH, mH, l), _F(IR[:, :, 0:2]), Ind[I_, I_, -1]),
        ((1, 1, lH), sub(3, 3, 2), Ind[0, 0, I_]), ((n, 1, lH), sub(1, 3, 2), Ind[-1, 0, I_]),
        ((1, m, lH), sub(3, 1, 2), Ind[0, -1, I_]), ((n, m, lH), sub(1, 1, 2), Ind[-1, -1, I_]),
        ((1, mH, 1), sub(3, 2, 3), Ind[0, I_, 0]), ((n, mH, 1), sub(1, 2, 3), Ind[-1, I_, 0]),
        ((1, mH, l), sub(3, 2, 1), Ind[0, I_, -1]), ((n, mH, l), sub(1, 2, 1), Ind[-1, I_, -1]),
        ((nH, 1, 1), sub(2, 3, 3), Ind[I_, 0, 0]), ((nH, m, 1), sub(2, 1, 3), Ind[I_, -1, 0]),
        ((nH, 1, l), sub(2, 3, 1), Ind[I_, 0, -1]), ((nH, m, l), sub(2, 1, 1), Ind[I_, -1, -1]),
        ((1, 1, 1), _F(IR[1:3, 1:3, 1:3]), Ind[0, 0, 0]), ((n, 1, 1), _F(IR[0:2, 1:3, 1:3]), Ind[-1, 0, 0]),
        ((1, m, 1), _F(IR[1:3, 0:2, 1:3]), Ind[0, -1, 0]), ((n, m, 1), _F(IR[0:2, 0:2, 1:3]), Ind[-1, -1, 0]),
        ((1, 1, l), _F(IR[1:3, 1:3, 0:2]), Ind[0, 0, -1]), ((n, 1, l), _F(IR[0:2, 1:3, 0:2]), Ind[-1, 0, -1]),
        ((1, m, l), _F(IR[1:3, 0:2, 0:2]), Ind[0, -1, -1]), ((n, m, l), _F(IR[0:2, 0:2, 0:2]), Ind[-1, -1, -1]),
    ]
    # entriesSparseG3D samples the same sources in the same order
    return [(ci(*p) + s, s, ci(*p) + s, _F(np.atleast_1d(r))) for p, s, r in spec]


def classes(n, m, l=1):
    return classes_2d(n, m) if l == 1 else classes_3d(n, m, l)


# ---- assembly -----------------------------------------------------------------------------------------------------
def create_indices(row, col, val):
    """createIndices (src/Functions.jl:7-29), 1-based"""
    row = np.atleast_1d(row)
    Row = np.kron(row, np.ones(len(col), dtype=np.int64))
    Col = np.kron(np.ones(len(row), dtype=np.int64), col) + Row
    Val = np.kron(np.ones(len(row)), val)
    return Row, Col, Val


def build(rows, n, m, l=1, nu=None, k=None, per_class=None):
    """As, AG (and Msp = As + k^2 AG diag(nu) when nu is given) as CSC, per-class a_c, ag_c, sigma[nclass, 3]
    (max, second smallest, min), row_class[N] and cancel[nclass] = |G[S,S]|_2 / |a_c G[S,S]|, the factor by which an error of
    a_c can grow in the AG row.  per_class(c, R, Gs, U, s), if given, sees every class's rows
    R = G[S_c, :], Gs = G[S_c, complement of S_c] and its SVD before they are dropped."""
    N = n * m * l
    cls = classes(n, m, l)
    ra, ca, va, vg = [], [], [], []
    row_class = np.full(N, -1, dtype=np.int64)
    sig, avals, agvals, cancel = [], [], [], []
    for c, (sA, ind, sG, rws) in enumerate(cls):
        sA0 = np.asarray(sA) - 1
        comp = np.setdiff1d(np.arange(N), sA0)
        R = rows(sA0)
        Gs = R[:, comp]
        U, s, _ = np.linalg.svd(Gs, full_matrices=False)
        if per_class is not None:
            per_class(c, R, Gs, U, s)
        a = U[:, -1].conj()                                         # U[:, end]'
        sG0 = np.asarray(sG) - 1
        Gss = rows(sG0)[:, sG0]
        ag = a @ Gss                                                # Values[c] * Entries[c]
        cancel.append(np.linalg.norm(Gss, 2) / np.linalg.norm(ag))  # |a| = 1
        sig.append((s[0], s[-2], s[-1]))
        avals.append(a)
        agvals.append(ag)
        R, Cc, V = create_indices(rws, ind, a)
        _, _, Vg = create_indices(rws, ind, ag)
        ra.append(R); ca.append(Cc); va.append(V); vg.append(Vg)
        row_class[np.asarray(rws) - 1] = c
    R = np.concatenate(ra) - 1
    Cc = np.concatenate(ca) - 1
    As = sp.coo_matrix((np.concatenate(va), (R, Cc)), shape=(N, N)).tocsc()
    AG = sp.coo_matrix((np.concatenate(vg), (R, Cc)), shape=(N, N)).tocsc()
    out = dict(As=As, AG=AG, a=avals, ag=agvals, sigma=np.array(sig), row_class=row_class, classes=cls,
               cancel=np.array(cancel))
    if nu is not None:
        out["Msp"] = (As + k ** 2 * (AG @ sp.diags(np.asarray(nu, float)))).tocsc()
    return out


def pattern(n, m, l=1):
    """(rowptr, col, row_class) of the reference's assembly, values all ones"""
    N = n * m * l
    R, Cc = [], []
    row_class = np.full(N, -1, dtype=np.int64)
    for c, (_, ind, _, rws) in enumerate(classes(n, m, l)):
        r, cc, _ = create_indices(rws, ind, np.ones(len(ind)))
        R.append(r); Cc.append(cc)
        row_class[np.asarray(rws) - 1] = c
    A = sp.coo_matrix((np.ones(sum(len(r) for r in R)), (np.concatenate(R) - 1, np.concatenate(Cc) - 1)), shape=(N, N)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64), row_class, A.nnz
