"""Long-double reference of the TRANSPOSED block-tridiagonal sweeps (test infrastructure, not product code; no GPU).

With the blocks of tests/blocktri_ref.py (D_k, L_k in block row k column k-1, U_k in block row k column k+1, and the
inverses S_k^{-1} of the elimination of Msp itself), Msp^T x = w is solved by

    forward    z_k = S_k^{-T} (w_k - U_{k-1}^T z_{k-1})                       k = 0 .. K-1
    backward   x_{K-1} = z_{K-1},   x_k = z_k - S_k^{-T} (L_{k+1}^T x_{k+1})    k = K-2 .. 0

`solve_t_ld` runs them in long double on the blocks given, in the manner of `blocktri_cases.solve_ld`; `precond_t` and
`precond_h` are the transposed and the adjoint preconditioner As^T Msp^{-T} and conj(. conj) built on it."""
import functools

import numpy as np

import blocktri_ref as bt

LD = np.clongdouble

# left-preconditioned GMRES(20) to 1e-6, rhs = -(M u_inc - u_inc): (preconditioned, plain) steps per op, from the oracle
# (tests/test_blocktri_transpose_cpu.py reproduces them)
PHYSICAL = {
    ("gv3", (16, 16, 16)): {"N": (3, 5), "T": (3, 5), "H": (3, 6)},
    ("trap", (41, 41, 1)): {"N": (4, 8), "T": (3, 8), "H": (3, 9)},
}


@functools.lru_cache(maxsize=None)
def oracle_solves(kind, dims):
    """{"N" | "T" | "H": (steps with the preconditioner of that op, steps without)} and the right-hand side, from the oracle
    operator, tests/adjoint_ref.py and scipy's LU of Msp and of Msp.T on the pair of `blocktri_ref.ref_pair`"""
    import scipy.sparse.linalg as spla
    from oracle import lsfc_oracle as o
    import adjoint_ref as ar
    n = dims[0]
    if kind == "gv3":
        h = 1.0 / n
        x = -0.5 + h * np.arange(n)
        k = 1.0 / h
        X, Y, Z = o.grid3d(x, x, x)
        Mo = o.build_fast_convolution3d(x, x, x, X, Y, Z, h, k, bt.nu3)
    else:
        h = 1.0 / (n - 1)
        x = -0.5 + h * np.arange(n)
        k = 1.0 / h
        X, Y = o.grid2d(x, x)
        Mo = o.build_fast_convolution(x, x, h, k, bt.nu2, quadRule="trapezoidal")
    u_inc = np.exp(1j * k * X).ravel()
    Msp, As = bt.ref_pair(kind, dims)
    lu, luT = spla.splu(Msp.tocsc()), spla.splu(Msp.T.tocsc())
    R = ar.ref_of_oracle(Mo)
    N = Msp.shape[0]
    rhs = -(o.mul(Mo, u_inc) - u_inc)
    AsT = As.T.tocsr()
    PT = lambda v: AsT @ luT.solve(v)                      # noqa: E731
    ops = {"N": (lambda v: o.mul(Mo, v), lambda v: lu.solve(As @ v)), "T": (R.T, PT), "H": (R.H, lambda v: np.conj(PT(np.conj(v))))}
    counts = {}
    for name, (A, P) in ops.items():
        _, with_p = o.gmres(np.zeros(N, complex), A, rhs, Pl=P, reltol=1e-6, restart=20)
        _, plain = o.gmres(np.zeros(N, complex), A, rhs, reltol=1e-6, restart=20, maxiter=400)
        assert with_p.isconverged and plain.isconverged
        counts[name] = (int(with_p.iters), int(plain.iters))
    return counts, rhs


def solve_t_ld(Msp, Sinv, w):
    """x = Msp^{-T} w by the two transposed sweeps in long double: the sparse products as scatter-adds, the dense ones as
    long-double matrix products.  w: (N,) or (members, N); the result has w's shape, dtype clongdouble."""
    K = len(Sinv)
    b, blk = bt._blocks(Msp, K)
    W = np.atleast_2d(np.asarray(w)).astype(LD).T          # N x members
    Z = np.zeros_like(W)

    def sparse_mul_t(i, j, V):
        """block (i, j) of Msp, transposed, times V"""
        B = blk(i, j).tocoo()
        out = np.zeros_like(V)
        np.add.at(out, B.col, B.data.astype(LD)[:, None] * V[B.row])
        return out

    for k in range(K):
        T = W[k * b:(k + 1) * b].copy()
        if k:
            T -= sparse_mul_t(k - 1, k, Z[(k - 1) * b:k * b])                 # U_{k-1}^T z_{k-1}
        Z[k * b:(k + 1) * b] = Sinv[k].astype(LD).T @ T
    for k in range(K - 2, -1, -1):
        Z[k * b:(k + 1) * b] -= Sinv[k].astype(LD).T @ sparse_mul_t(k + 1, k, Z[(k + 1) * b:(k + 2) * b])   # L_{k+1}^T x_{k+1}
    return Z.T.reshape(np.shape(w))


def spmv_t_ld(As, X):
    """As^T x in long double for x of shape (N,) or (members, N)"""
    A = As.tocoo()
    V = np.atleast_2d(np.asarray(X)).astype(LD).T
    out = np.zeros_like(V)
    np.add.at(out, A.col, A.data.astype(LD)[:, None] * V[A.row])
    return out.T.reshape(np.shape(X))


def precond_t(Msp, As, Sinv, v):
    """As^T Msp^{-T} v in long double"""
    return spmv_t_ld(As, solve_t_ld(Msp, Sinv, v))


def precond_h(Msp, As, Sinv, v):
    return np.conj(precond_t(Msp, As, Sinv, np.conj(np.asarray(v))))
