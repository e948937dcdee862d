"""Test infrastructure for the device preconditioner apply (csrc/precond.hip, csrc/trisolve.hip): a high-precision
restatement of the operator lsfc_precond_create / lsfc_precond_apply define (include/lsfc.h), and a generator of triangular factors whose
dependency levels have prescribed sizes, so that a test can steer the launch schedule into each kind of segment.

    apply_ref(As, L, U, row_gather, col_scatter, row_scale, b, dtype)
        y = As b;  y0[k] = row_scale[g_k] y[g_k] with g_k = row_gather[k];  z = L^-1 y0;  w = U^-1 z;
        out[col_scatter[k]] = w[k] -- row by row in `dtype` (np.clongdouble: the reference; np.complex128: a plain
        double-precision baseline of the same arithmetic)

    make_factor(levels, lower, seed)
        levels: one (rows, off-diagonal entries per row) or (rows, entries, window) per dependency level, level 0 first.
        A row of level l > 0 depends on one row of level l - 1 and on entries - 1 further distinct rows of levels < l
        (drawn from the `window` rows sorted last before level l when a window is given: dense coupling to the rows
        just before).  Rows are numbered in a random topological order, not level by level.  Values are complex; the
        off-diagonal moduli of a row sum to at most 0.5 |diagonal|.  U (lower=False) is the mirror image of L."""
import heapq

import numpy as np
import scipy.sparse as sp

assert np.finfo(np.longdouble).nmant > 52, "the reference needs an extended-precision long double"


def _csr_rows(A, dtype):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr, A.indices, A.data.astype(dtype)


def _trsv(A, b, lower, dtype):
    ptr, col, val = _csr_rows(A, dtype)
    N = b.size
    x = np.zeros(N, dtype=dtype)
    for r in (range(N) if lower else range(N - 1, -1, -1)):
        c, v = col[ptr[r]:ptr[r + 1]], val[ptr[r]:ptr[r + 1]]
        d = v[c == r]
        assert d.size == 1 and d[0] != 0, f"row {r}: zero or missing diagonal"
        off = c != r
        assert np.all(c[off] < r) if lower else np.all(c[off] > r), f"row {r}: entry on the wrong side of the diagonal"
        x[r] = (b[r] - np.sum(v[off] * x[c[off]])) / d[0]
    return x


def apply_ref(As, L, U, row_gather, col_scatter, row_scale, b, dtype=np.clongdouble):
    """v <- Msp^-1 (As v) through the factors, as include/lsfc.h defines it; None for an identity map / unit scale"""
    N = L.shape[0]
    ptr, col, val = _csr_rows(As, dtype)
    bb = np.asarray(b).astype(dtype)
    y = np.array([np.sum(val[ptr[r]:ptr[r + 1]] * bb[col[ptr[r]:ptr[r + 1]]]) for r in range(N)], dtype=dtype)
    g = np.arange(N) if row_gather is None else np.asarray(row_gather)
    y0 = y[g] if row_scale is None else y[g] * np.asarray(row_scale, dtype=np.float64)[g].astype(dtype)
    w = _trsv(U, _trsv(L, y0, True, dtype), False, dtype)
    out = np.empty(N, dtype=dtype)
    out[np.arange(N) if col_scatter is None else np.asarray(col_scatter)] = w
    return out


def levels_of(F, lower):
    """dependency level of every row of a triangular factor, as the solve's scheduler computes it"""
    F = sp.csr_matrix(F)
    N = F.shape[0]
    lv = np.zeros(N, dtype=np.int64)
    for r in (range(N) if lower else range(N - 1, -1, -1)):
        c = F.indices[F.indptr[r]:F.indptr[r + 1]]
        c = c[c != r]
        lv[r] = lv[c].max() + 1 if c.size else 0
    return lv


def make_factor(levels, lower=True, seed=0):
    rng = np.random.default_rng(seed)
    spec = [(int(t[0]), int(t[1]), t[2] if len(t) > 2 else None) for t in levels]
    N = sum(r for r, _, _ in spec)
    # dependencies, rows identified by their position in level order
    first = np.cumsum([0] + [r for r, _, _ in spec])
    deps = []
    for l, (rows, k, window) in enumerate(spec):
        assert rows >= 1
        if l == 0:
            assert k == 0, "rows of level 0 depend on nothing"
            deps += [np.zeros(0, dtype=np.int64)] * rows
            continue
        assert k >= 1, f"level {l}: a row needs an entry in level {l - 1}"
        lo = 0 if window is None else max(0, first[l] - window)
        for _ in range(rows):
            prev = rng.integers(first[l - 1], first[l])
            pool = np.setdiff1d(np.arange(lo, first[l]), [prev])
            assert pool.size >= k - 1, f"level {l}: {k} entries per row, only {pool.size + 1} earlier rows to draw from"
            deps.append(np.concatenate([[prev], rng.choice(pool, k - 1, replace=False)]).astype(np.int64))
    # a random topological order (Kahn's algorithm with random priorities)
    waiting = np.array([d.size for d in deps])
    users = [[] for _ in range(N)]
    for i, d in enumerate(deps):
        for j in d:
            users[j].append(i)
    prio = rng.permutation(N)
    heap = [(prio[i], i) for i in range(N) if waiting[i] == 0]
    heapq.heapify(heap)
    number = np.empty(N, dtype=np.int64)
    nxt = 0
    while heap:
        _, i = heapq.heappop(heap)
        number[i] = nxt
        nxt += 1
        for u in users[i]:
            waiting[u] -= 1
            if waiting[u] == 0:
                heapq.heappush(heap, (prio[u], u))
    assert nxt == N
    # values: diagonal of modulus 1..2, off-diagonal moduli summing to 0.05..0.5 of it
    rows, cols, vals = [], [], []
    for i, d in enumerate(deps):
        diag = rng.uniform(1.0, 2.0) * np.exp(2j * np.pi * rng.uniform())
        rows.append(number[i]); cols.append(number[i]); vals.append(diag)
        if d.size:
            m = rng.uniform(0.2, 1.0, d.size)
            m *= rng.uniform(0.05, 0.5) * abs(diag) / m.sum()
            rows += [number[i]] * d.size
            cols += list(number[d])
            vals += list(m * np.exp(2j * np.pi * rng.uniform(size=d.size)))
    rows, cols = np.asarray(rows), np.asarray(cols)
    if not lower:
        rows, cols = N - 1 - rows, N - 1 - cols
    F = sp.csr_matrix((np.asarray(vals, dtype=np.complex128), (rows, cols)), shape=(N, N))
    F.sort_indices()
    return F
