"""Host restatement of the partial row pivoting of csrc/blocktri_factor.hip and the inputs that need it (test infrastructure,
not product code; no GPU).

Pivot rule, as the device follows it: at elimination step p the candidates are rows p .. b-1 of column p (the rows that
have not been pivot rows yet); the pivot is the candidate with the largest x*x + y*y in fp64; on a tie the lowest row.
In-place Gauss-Jordan with these interchanges inverts Pi A; A^{-1} = (Pi A)^{-1} Pi, so the columns of the in-place result
are put back once at the end.

`permuted(shape, seed)`: a synthetic pair of tests/blocktri_cases.py with one random row permutation Pi_k applied to the
whole block row k of both matrices.  Rows move intact, so every row stays a sorted CSR row inside the three block
diagonals and the two matrices still share a pattern.  By induction S'_k = Pi_k S_k: the same condition number (2 to 3),
and Msp'^{-1} As' = Msp^{-1} As."""
import functools

import numpy as np
import scipy.sparse as sp

import blocktri_cases as bc

# (b, K, pattern): the boundary each one sits on is in DESIGN.md, "Shape suite"
PERMUTED_SHAPES = [
    (2, 3, "scattered"),                                   # smallest block with an interchange
    (31, 3, "scattered"), (32, 3, "scattered"), (33, 3, "scattered"),      # NB: last panel narrower than 32
    (64, 3, "scattered"), (65, 3, "ragged"),               # a second and third panel, pivots from later panels
    (97, 3, "scattered"),                                  # first size past the walk kernel
    (257, 2, "ragged"),                                    # 65th workgroup of the row moves (four columns each), one column
    (1025, 2, "scattered"),                                # many panels, one-column last panel; a second row per thread of the panel kernel
]
# seed of synth and of the permutations, per block size: chosen so that Gauss-Jordan without pivoting breaks down on the
# permuted pair (tests/test_blocktri_pivot_cpu.py asserts it)
SEEDS = {2: 18, 31: 31, 32: 32, 33: 33, 64: 64, 65: 65, 97: 97, 257: 257, 1025: 1025}


def gauss_jordan_partial(A):
    """in-place Gauss-Jordan inversion with partial row pivoting by the rule above;
    (inverse, perm, smallest chosen |pivot| / max|A|), perm[i] = row of A that became pivot row i"""
    A = np.array(A, dtype=np.complex128)
    b = A.shape[0]
    amax = np.abs(A).max()
    perm = np.arange(b)
    worst = np.inf
    with np.errstate(all="ignore"):
        for p in range(b):
            cand = A[p:, p]
            q = p + int(np.argmax(cand.real * cand.real + cand.imag * cand.imag))      # the first of equal maxima
            if q != p:
                A[[p, q], :] = A[[q, p], :]
                perm[[p, q]] = perm[[q, p]]
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
    out = np.empty_like(A)
    out[:, perm] = A                                       # (Pi A)^{-1} Pi: column perm[i] of the inverse is column i
    return out, perm, float(worst)


def pivots_partial(A):
    """(perm, smallest chosen |pivot| / max|A|) of the same rule by LU alone: rows >= p of column p are the same in
    Gauss-Jordan and in LU at step p, and the update of the trailing block is a third of the work"""
    A = np.array(A, dtype=np.complex128)
    b = A.shape[0]
    amax = np.abs(A).max()
    perm = np.arange(b)
    worst = np.inf
    with np.errstate(all="ignore"):
        for p in range(b):
            cand = A[p:, p]
            q = p + int(np.argmax(cand.real * cand.real + cand.imag * cand.imag))
            if q != p:
                A[[p, q], :] = A[[q, p], :]
                perm[[p, q]] = perm[[q, p]]
            piv = A[p, p]
            worst = min(worst, abs(piv) / amax)
            A[p + 1:, p + 1:] -= np.outer(A[p + 1:, p], A[p, p + 1:] / piv)
    return perm, float(worst)


def permute_block_rows(A, perms):
    """row k b + i of the result is row k b + perms[k][i] of A (CSR, rows intact)"""
    b = perms[0].size
    idx = np.concatenate([k * b + p for k, p in enumerate(perms)])
    B = sp.csr_matrix(A)[idx, :]
    B.sort_indices()
    return sp.csr_matrix((B.data, B.indices.astype(np.int64), B.indptr.astype(np.int64)), shape=B.shape)


@functools.lru_cache(maxsize=None)
def permuted(shape, seed):
    """(Msp', As', [Pi_k], Msp, As): the pair of bc.synth(b, K, pattern, seed) with block row k permuted by Pi_k (row i of
    block row k of Msp' is row Pi_k[i] of block row k of Msp), and the pair itself; computed once per process, read only"""
    b, K, pattern = shape
    Msp, As = bc.synth(b, K, pattern, seed)
    rng = np.random.default_rng(seed + 1000)
    perms = [rng.permutation(b) for _ in range(K)]
    return permute_block_rows(Msp, perms), permute_block_rows(As, perms), perms, Msp, As


def case(shape):
    return permuted(shape, SEEDS[shape[0]])


# ---- planted pivots (the construction of tests/test_gpu_blocktri_shapes.py, restated) ----------------------------------

PLANT_B, PLANT_K, PLANT_SMAX = 70, 3, 50.0


def planted(eps, second=False):
    """(Msp, As), 3 blocks of 70 rows.  U_0 is empty, so S_1 = D_1 exactly; D_1 = smax I except rows and columns 45, 46,
    which hold smax [[eps, 1], [1, eps]]: Gauss-Jordan without pivoting meets the pivot eps smax at row 45 of block 1
    (second 32-column panel), max|S_1| = smax; with partial pivoting rows 45 and 46 change places and nothing else moves.
    `second`: row 3 of block 2 keeps only a diagonal of 1e-12."""
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


def from_dense(Md, Ad, stored):
    """(Msp, As) as CSR of the pattern `stored` (boolean mask, row by row, columns ascending)"""
    rows, cols = np.nonzero(stored)
    indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int64)
    csr = lambda A: sp.csr_matrix((A[rows, cols], cols.astype(np.int64), indptr.copy()), shape=A.shape)   # noqa: E731
    return csr(np.asarray(Md, dtype=np.complex128)), csr(np.asarray(Ad, dtype=np.complex128))


def tie_pair(b=40):
    """(Msp, As), one block of b rows: every entry of the first column is one of 1, -1, i, -i (modulus exactly 1, x*x + y*y
    exactly 1), elsewhere the rows are dominant (diagonal 8, a few entries of modulus <= 0.5): all b candidates of the first
    step tie, and the rule takes row 0"""
    rng = np.random.default_rng(b)
    Md = np.zeros((b, b), dtype=np.complex128)
    stored = np.eye(b, dtype=bool)
    for i in range(b):
        cols = rng.choice(np.arange(1, b), 4, replace=False)
        stored[i, cols] = True
        Md[i, cols] = 0.5 * np.exp(2j * np.pi * rng.random(4)) * rng.random(4)
    Md[np.arange(1, b), np.arange(1, b)] = 8.0 * np.exp(2j * np.pi * rng.random(b - 1))
    stored[:, 0] = True
    Md[:, 0] = np.array([1.0, -1.0, 1j, -1j])[rng.integers(0, 4, b)]
    Ad = np.where(stored, rng.standard_normal((b, b)) + 1j * rng.standard_normal((b, b)), 0.0)
    return from_dense(Md, Ad, stored)


def singular_pair(b=40, K=2):
    """(Msp, As) of bc.synth(b, K, "scattered") with rows 5 and 9 of block row 1 made identical in Msp, couplings L_1
    included (As likewise, so the two keep one pattern): S_1 has two identical rows and is singular under any pivoting"""
    Msp, As = bc.synth(b, K, "scattered", seed=b + 1)
    Md, Ad = Msp.toarray(), As.toarray()
    stored = Md != 0
    r0, r1 = b + 5, b + 9
    stored[r1] = stored[r0]
    Md[r1], Ad[r1] = Md[r0], Ad[r0]
    return from_dense(Md, Ad, stored)
