"""numpy restatement of the block-tridiagonal elimination of Msp (test infrastructure, not product code).

With the slowest grid axis as block index Msp is block tridiagonal, K blocks of b rows:

    S_0 = D_0,   S_k = D_k - L_k S_{k-1}^{-1} U_{k-1}
    forward   z_k = S_k^{-1} (w_k - L_k z_{k-1})
    backward  x_{K-1} = z_{K-1},   x_k = z_k - S_k^{-1} (U_k x_{k+1})

`eliminate` returns the explicit inverses (np.linalg.inv, partial pivoting), `solve` runs the two sweeps.
`ref_pair` builds (Msp, As) of the cases of tests/test_gpu_sparsify.py from the restatement alone (no device)."""
import numpy as np
import scipy.sparse as sp

from oracle import lsfc_oracle as o
import sparsify_ref as ref


def nu2(X, Y):                                             # examples/example.jl:48
    return 0.3 * np.exp(-40 * (X ** 2 + Y ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48)


def nu3(X, Y, Z):                                          # examples/example3D.jl:43
    return 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48)


def ref_pair(kind, dims):
    """(Msp, As) as CSR from tests/sparsify_ref.py, the grids and wave numbers of test_gpu_sparsify.case"""
    n = dims[0]
    if kind == "trap":
        h = 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        k = 1.0 / h
        X, Y = o.grid2d(x, x)
        D0 = o.reference_vals_trap_rule()[1][0]
        r = ref.build(ref.direct_rows(k, X, Y, D0, h), n, n, nu=nu2(X, Y), k=k)
    else:
        n, m, l = dims
        h = 1.0 / n
        x, y, z = (-0.5 + h * np.arange(v) for v in (n, m, l))
        k = 1.0 / h
        X, Y, Z = o.grid3d(x, y, z)
        box = abs(x[-1] - x[0]) + h
        r = ref.build(ref.gv3d_rows(n, m, l, box, k), n, m, l, nu=nu3(X, Y, Z), k=k)
    return sp.csr_matrix(r["Msp"]), sp.csr_matrix(r["As"])


def in_band(rowptr, col, K):
    """every stored entry lies in block row k, block column k-1, k or k+1"""
    N = len(rowptr) - 1
    b = N // K
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    return N % K == 0 and bool(np.all(np.abs(np.asarray(col) // b - rows // b) <= 1))


def _blocks(Msp, K):
    Msp = sp.csr_matrix(Msp)
    N = Msp.shape[0]
    b = N // K
    assert b * K == N
    blk = lambda i, j: Msp[i * b:(i + 1) * b, j * b:(j + 1) * b]          # noqa: E731
    return b, blk


def eliminate(Msp, K):
    """[S_k^{-1}] (dense b x b), k = 0 .. K-1"""
    b, blk = _blocks(Msp, K)
    Sinv = []
    for k in range(K):
        S = blk(k, k).toarray()
        if k:
            S = S - blk(k, k - 1) @ (Sinv[-1] @ blk(k - 1, k).toarray())
        Sinv.append(np.linalg.inv(S))
    return Sinv


def solve(Msp, Sinv, w):
    """x = Msp^{-1} w by the two sweeps"""
    K = len(Sinv)
    b, blk = _blocks(Msp, K)
    w = np.asarray(w, dtype=np.complex128)
    z = np.empty_like(w)
    for k in range(K):
        t = w[k * b:(k + 1) * b].copy()
        if k:
            t -= blk(k, k - 1) @ z[(k - 1) * b:k * b]
        z[k * b:(k + 1) * b] = Sinv[k] @ t
    for k in range(K - 2, -1, -1):
        z[k * b:(k + 1) * b] -= Sinv[k] @ (blk(k, k + 1) @ z[(k + 1) * b:(k + 2) * b])
    return z


def gauss_jordan_nopivot(A):
    """in-place Gauss-Jordan inversion without pivoting; (inverse, smallest |pivot| / max|A|)"""
    A = np.array(A, dtype=np.complex128)
    amax = np.abs(A).max()
    worst = np.inf
    for p in range(A.shape[0]):
        piv = A[p, p]
        worst = min(worst, abs(piv) / amax)
        col = A[:, p].copy()
        A[p, :] /= piv
        A[p, p] = 1.0 / piv
        row = A[p, :].copy()
        col[p] = 0.0
        A[:, p] = 0.0
        A[p, :] = row
        A -= np.outer(col, row)
    return A, worst
