"""Synthetic block-tridiagonal inputs for csrc/blocktri_factor.hip and a long-double reference of the two sweeps of csrc/blocktri_sweep.hip (test
infrastructure, not product code; no GPU).

The physical cases of tests/test_gpu_precond_blocktri.py have six block sizes and the 9- / 27-point stencil only.  The
C entry point takes any block-tridiagonal CSR pair, and the block size b selects tile counts, masks and kernels, so the
shapes here sit on those boundaries (`SHAPES`) and the patterns are not stencils:

    "scattered"  in each of the three blocks of a row min(6, b) distinct random columns, not banded on purpose (a banded
                 pattern gives inverses that decay into the float-denormal range at large b, this one does not)
    "dense"      all three blocks full: a column of the upper coupling holds b entries
    "ragged"     scattered; a quarter of the rows without lower coupling, a quarter without upper coupling, a few rows
                 with the diagonal as their only entry of the diagonal block, and (K >= 3) one interior pair of coupling
                 blocks L_k, U_{k-1} completely empty
    "blockdiag"  no couplings at all (K > 1 and not one entry in any U_k)

Values are random complex; the diagonal of Msp is 2 (sum of |off-diagonal| of the row) e^{i theta} (1 where a row has
nothing but its diagonal), so Msp is strictly diagonally dominant by rows and so is every Schur complement: Gauss-Jordan
without pivoting is safe and cond(S_k) is 2 to 3."""
import functools

import numpy as np
import scipy.sparse as sp

import blocktri_ref as bt

LD = np.clongdouble
DEGREE = 6                                                 # stored columns per row and block of the scattered patterns

# (b, K, pattern): the boundary each one sits on is in DESIGN.md, "Shape suite"
SHAPES = [
    (1, 5, "scattered"),                                   # scalar tridiagonal, one panel of one column
    (16, 3, "scattered"), (17, 3, "scattered"),            # AP_ROWS inside the walk kernel
    (31, 3, "scattered"), (32, 3, "scattered"), (33, 3, "scattered"),      # NB: narrow last panel; first trailing update
    (64, 3, "dense"),                                      # long columns of U; BB_ROWS
    (65, 3, "ragged"),                                     # BB_ROWS + 1, empty couplings
    (96, 3, "scattered"), (97, 3, "scattered"), (98, 3, "scattered"),      # WALK_B; first launches per step; odd / even row pairs
    (129, 2, "scattered"),                                 # second 128-row tile of the float group product, one row
    (257, 2, "ragged"),                                    # second workgroup of the panel kernel, one thread; 81 trail tiles
    (70, 2, "blockdiag"),                                  # no upper coupling anywhere with K > 1
    (1023, 2, "scattered"), (1024, 2, "scattered"), (1025, 2, "scattered"),    # group product: 32 -> 64 column ranges
    (2048, 2, "scattered"), (2049, 2, "scattered"),        # second staging chunk of one entry, with couplings; 128 column ranges
]


def shape_id(shape):
    b, K, pattern = shape
    return f"b{b}-K{K}-{pattern}"


def _block_columns(b, pattern, rng):
    """(rows, columns) inside one b x b block"""
    if pattern == "dense":
        r, c = np.divmod(np.arange(b * b), b)
        return r, c
    d = min(DEGREE, b)
    return np.repeat(np.arange(b), d), np.concatenate([rng.choice(b, d, replace=False) for _ in range(b)])


def synth(b, K, pattern, seed):
    """(Msp, As): CSR of one sorted pattern inside the three block diagonals of K blocks of b rows, the diagonal stored"""
    assert pattern in ("scattered", "dense", "ragged", "blockdiag")
    rng = np.random.default_rng(seed)
    N = b * K
    ragged = pattern == "ragged"
    if ragged:
        no_lower = np.zeros(N, dtype=bool)
        no_lower[rng.choice(N, N // 4, replace=False)] = True
        no_upper = np.zeros(N, dtype=bool)
        no_upper[rng.choice(N, N // 4, replace=False)] = True
        diag_only = np.zeros(N, dtype=bool)
        diag_only[rng.choice(N, max(1, N // 16), replace=False)] = True
        empty = (K // 2, K // 2 + 1) if K >= 3 else None   # no coupling between these two blocks, in either direction
    rows, cols = [np.arange(N)], [np.arange(N)]
    for k in range(K):
        for kk in (k - 1, k, k + 1):
            if kk < 0 or kk >= K or (pattern == "blockdiag" and kk != k):
                continue
            r, c = _block_columns(b, pattern, rng)
            if ragged:
                drop = (no_lower, diag_only, no_upper)[kk - k + 1][k * b:(k + 1) * b]
                keep = ~drop[r] if (min(k, kk), max(k, kk)) != empty else np.zeros(r.size, dtype=bool)
                r, c = r[keep], c[keep]
            rows.append(k * b + r)
            cols.append(kk * b + c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    pat = sp.csr_matrix((np.ones(rows.size), (rows, cols)), shape=(N, N))
    pat.sum_duplicates()
    pat.sort_indices()
    indptr, indices = pat.indptr.astype(np.int64), pat.indices.astype(np.int64)
    on_diag = np.repeat(np.arange(N), np.diff(indptr)) == indices
    assert on_diag.sum() == N

    def values():
        return rng.standard_normal(indices.size) + 1j * rng.standard_normal(indices.size)

    m_val, a_val = values(), values()
    m_val[on_diag] = 0.0
    off = np.add.reduceat(np.abs(m_val), indptr[:-1])      # every row is non-empty: it holds its diagonal
    m_val[on_diag] = np.where(off > 0.0, 2.0 * off, 1.0) * np.exp(2j * np.pi * rng.random(N))
    Msp = sp.csr_matrix((m_val, indices.copy(), indptr.copy()), shape=(N, N))
    As = sp.csr_matrix((a_val, indices.copy(), indptr.copy()), shape=(N, N))
    return Msp, As


@functools.lru_cache(maxsize=None)
def built(shape):
    """(Msp, As, [S_k^{-1}] of blocktri_ref.eliminate) of an entry of SHAPES, computed once per process; read only"""
    b, K, pattern = shape
    Msp, As = synth(b, K, pattern, seed=b)
    return Msp, As, bt.eliminate(Msp, K)


def right_hand_sides(N, count, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((count, N)) + 1j * rng.standard_normal((count, N))


def schur_blocks(Msp, K):
    """[S_k] (dense b x b, fp64): S_0 = D_0, S_k = D_k - L_k S_{k-1}^{-1} U_{k-1} with np.linalg.inv (partial pivoting)"""
    b, blk = bt._blocks(Msp, K)
    S = []
    for k in range(K):
        Sk = blk(k, k).toarray()
        if k:
            Sk = Sk - blk(k, k - 1) @ (np.linalg.inv(S[-1]) @ blk(k - 1, k).toarray())
        S.append(Sk)
    return S


def min_pivot_ratio(Msp, K):
    """smallest |pivot| / max|S_k| of Gauss-Jordan without pivoting over all Schur blocks"""
    return min(bt.gauss_jordan_nopivot(S)[1] for S in schur_blocks(Msp, K))


def smallest_part(blocks):
    """smallest non-zero |real or imaginary part| of any block"""
    smallest = np.inf
    for S in blocks:
        parts = np.abs(np.concatenate([S.real.ravel(), S.imag.ravel()]))
        smallest = min(smallest, parts[parts > 0].min())
    return float(smallest)


def solve_ld(Msp, Sinv, w):
    """The two sweeps of blocktri_ref.solve in long double on the blocks given: the sparse products as scatter-adds, the
    dense ones as long-double matrix products.  w: (N,) or (members, N); the result has w's shape, dtype clongdouble."""
    K = len(Sinv)
    b, blk = bt._blocks(Msp, K)
    W = np.atleast_2d(np.asarray(w)).astype(LD).T          # N x members
    Z = np.zeros_like(W)

    def sparse_mul(i, j, V):
        B = blk(i, j).tocoo()
        out = np.zeros_like(V)
        np.add.at(out, B.row, B.data.astype(LD)[:, None] * V[B.col])
        return out

    for k in range(K):
        T = W[k * b:(k + 1) * b].copy()
        if k:
            T -= sparse_mul(k, k - 1, Z[(k - 1) * b:k * b])
        Z[k * b:(k + 1) * b] = Sinv[k].astype(LD) @ T
    for k in range(K - 2, -1, -1):
        Z[k * b:(k + 1) * b] -= Sinv[k].astype(LD) @ sparse_mul(k, k + 1, Z[(k + 1) * b:(k + 2) * b])
    return Z.T.reshape(np.shape(w))


def elementwise_err(x, ref):
    """max|x - ref| / max|ref|: one wrong row cannot hide in it as it can in a norm"""
    x, ref = np.asarray(x).ravel(), np.asarray(ref).ravel()
    return float(np.max(np.abs(x - ref)) / np.max(np.abs(ref)))
