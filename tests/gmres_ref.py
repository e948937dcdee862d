"""Test infrastructure for the device GMRES (csrc/gmres.hip, BLAS-1 kernels in csrc/krylov_blas.hip): a long-double
restatement of its solve() over a diagonal operator, and the problems that drive its code paths.

    gmres_ref(b, a, pl, counts, restart, maxiter, reltol, abstol, orth, x0, initially_zero, dtype)
        restarted, left-preconditioned GMRES for  diag(pl) diag(a) x = diag(pl) b  with the control flow of solve():
        init / initially_zero, expand then the left preconditioner, MGS / CGS / DGKS (the `nrm < proj / sqrt(2)` loop
        with its 8-pass guard, corrections added into the Hessenberg column), the null-vector residual estimate, Givens
        least squares at restart or convergence, `current` kept across a restart, the mvps / iters accounting.
        A zero subdiagonal H[k+1,k] or a non-finite null-vector entry (an exhausted Krylov space) counts as convergence.

        Vectors are constant on GROUPS: group g stands for counts[g] equal entries, and every inner product is
        sum_g counts[g] conj(u_g) w_g.  With unit counts this is GMRES on full vectors; a few hundred groups state a
        problem of several million entries exactly.  a / pl: per-group diagonals (None: identity).

        Returns a dict: resnorm (per iteration), iters, mvps, converged, x (per group), passes (DGKS re-orthogonalisation
        passes per step), subdiag (H[k+1,k] per step), beta0, tol, cycle_beta (the beta of the cycle of every step).

    history_excess(h, ref)               how far a double-precision history strays from the reference, in units of
                                         what double rounding allows

    disc_spectrum(m, rho_max, seed)      lambda = 1 + rho e^{i theta}, rho <= rho_max: GMRES contracts by ~rho_max per step
    cluster_spectrum(m, spread, seed)    lambda within `spread` of 1: the Krylov basis loses orthogonality, DGKS corrects
    group_map(N, m, p)                   g(i) = (i p) mod m, p coprime to m: every block and every tail holds mixed groups
    group_counts(N, m, p)                entries per group of that map
    exhausted_problem(kind, ...)         N <= restart, or fewer distinct eigen-components than the restart length"""
import math

import numpy as np

assert np.finfo(np.longdouble).nmant > 52, "the reference needs an extended-precision long double"

ORTHS = ("MGS", "CGS", "DGKS")
DEFAULT_RELTOL = math.sqrt(2.220446049250313e-16)


def _givens(f, g, dtype):
    """LinearAlgebra.givensAlgorithm for complex f, g: [c s; -conj(s) c] [f; g] = [r; 0], c real"""
    real = np.longdouble if dtype == np.clongdouble else np.float64
    if g == 0:
        return real(1), dtype(0)
    if f == 0:
        return real(0), np.conj(g) / abs(g)
    af, ag = abs(f), abs(g)
    d = np.sqrt(af * af + ag * ag)
    return af / d, (f / af) * np.conj(g) / d


def _solve_least_squares(H, beta, k, dtype):
    """hessenberg.jl: Givens QR of the k x (k-1) Hessenberg block against beta e1, then the triangular solve"""
    width = k - 1
    A = H[:k, :width].copy()
    rhs = np.zeros(k, dtype=dtype)
    rhs[0] = beta
    for i in range(width):
        c, s = _givens(A[i, i], A[i + 1, i], dtype)
        top, bot = A[i, i:].copy(), A[i + 1, i:].copy()
        A[i, i:] = c * top + s * bot
        A[i + 1, i:] = -np.conj(s) * top + c * bot
        r0, r1 = rhs[i], rhs[i + 1]
        rhs[i], rhs[i + 1] = c * r0 + s * r1, -np.conj(s) * r0 + c * r1
    y = np.zeros(width, dtype=dtype)
    for i in range(width - 1, -1, -1):
        y[i] = (rhs[i] - np.sum(A[i, i + 1:width] * y[i + 1:])) / A[i, i]
    return y


def gmres_ref(b, a=None, pl=None, counts=None, restart=None, maxiter=None, reltol=None, abstol=0.0, orth="MGS", x0=None,
              initially_zero=False, dtype=np.clongdouble):
    assert orth in ORTHS
    b = np.asarray(b).astype(dtype)
    m = b.size
    real = np.longdouble if dtype == np.clongdouble else np.float64
    c = np.ones(m, dtype=real) if counts is None else np.asarray(counts, dtype=np.float64).astype(real)
    N = int(m if counts is None else np.sum(counts))
    a = None if a is None else np.asarray(a).astype(dtype)
    pl = None if pl is None else np.asarray(pl).astype(dtype)
    restart = min(20, N) if restart is None else int(restart)
    maxiter = N if maxiter is None else int(maxiter)
    reltol = DEFAULT_RELTOL if reltol is None else reltol
    x = np.zeros(m, dtype=dtype) if x0 is None else np.asarray(x0).astype(dtype)

    dot = lambda u, w: np.sum(c * np.conj(u) * w)                       # noqa: E731
    nrm2 = lambda w: np.sqrt(np.sum(c * (w.real * w.real + w.imag * w.imag)))  # noqa: E731
    A = (lambda v: v.copy()) if a is None else (lambda v: a * v)        # noqa: E731
    P = (lambda v: v) if pl is None else (lambda v: pl * v)             # noqa: E731

    V = np.zeros((restart + 1, m), dtype=dtype)
    H = np.zeros((restart + 1, restart), dtype=dtype)
    nullvec = np.ones(restart + 1, dtype=dtype)

    def init(skip_mv):
        w = P(b.copy() if skip_mv else b - A(x))
        beta = nrm2(w)
        V[0] = w / beta
        return beta

    def project(w, k):
        h = np.array([dot(V[i], w) for i in range(k)], dtype=dtype)
        return h, w - np.sum(h[:, None] * V[:k], axis=0)

    mvps = 1 if initially_zero else 0
    beta = init(initially_zero)
    beta0 = beta
    current, accumulator = beta, real(1)
    tol = max(reltol * float(current), abstol)
    k, iteration = 1, 0
    hist, passes, subdiag, betas = [], [], [], []
    while not (iteration >= maxiter or current <= tol):
        w = P(A(V[k - 1]))                                              # expand!, then ldiv!(Pl, w)
        mvps += 1
        npass = 0
        if orth == "MGS":
            h = np.zeros(k, dtype=dtype)
            for i in range(k):
                h[i] = dot(V[i], w)
                w = w - h[i] * V[i]
            nrm = nrm2(w)
        else:
            h, w = project(w, k)
            nrm = nrm2(w)
            if orth == "DGKS":
                proj = np.sqrt(np.sum(np.abs(h) ** 2))
                while nrm < proj / np.sqrt(real(2)) and npass < 8:
                    corr, w = project(w, k)
                    proj = np.sqrt(np.sum(np.abs(corr) ** 2))
                    h = h + corr
                    nrm = nrm2(w)
                    npass += 1
        passes.append(npass)
        subdiag.append(nrm)
        H[:k, k - 1] = h
        H[k, k - 1] = nrm
        if nrm != 0:
            V[k] = w / nrm
        # update_residual!; an exhausted Krylov space (zero subdiagonal, non-finite null-vector entry) has converged
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            nullvec[k] = -np.conj(np.sum(np.conj(nullvec[:k]) * H[:k, k - 1]) / nrm) if nrm != 0 else np.nan
        if nrm == 0 or not np.isfinite(nullvec[k]):
            current = real(0)
        else:
            accumulator += nullvec[k].real ** 2 + nullvec[k].imag ** 2
            current = beta / np.sqrt(accumulator)
        betas.append(beta)
        k += 1
        if k == restart + 1 or current <= tol:
            y = _solve_least_squares(H, beta, k, dtype)
            x = x + np.sum(y[:, None] * V[:k - 1], axis=0)
            k = 1
            if not current <= tol:
                beta = init(False)
                accumulator = real(1)
                nullvec[0] = 1
                mvps += 1
        hist.append(current)
        iteration += 1
    return {"resnorm": np.array(hist, dtype=np.float64), "resnorm_ld": np.array(hist), "iters": iteration, "mvps": mvps,
            "converged": bool(current <= tol), "x": x, "passes": passes, "subdiag": np.array(subdiag, dtype=np.float64),
            "beta0": float(beta0), "tol": tol, "cycle_beta": np.array(betas, dtype=np.float64)}


def history_excess(h, ref, rtol=1e-10, floor=1e-9):
    """max over the history entries where the reference residual is >= floor * beta0 of |h - ref| / allowed, allowed =
    rtol * ref + 1e-15 * beta0 * ref / cycle_beta.  The second term is the rounding of a double-precision iterate x
    (~eps |x|, |x| ~ beta0 here) that a restart turns into a relative error of the recomputed residual of its cycle; it is
    negligible in the first cycle.  Returns (excess, index of the worst entry); excess < 1 passes."""
    r = ref["resnorm"]
    h = np.asarray(h, dtype=np.float64)
    k = min(h.size, r.size)
    if k == 0:
        return 0.0, -1
    r, h, cb = r[:k], h[:k], ref["cycle_beta"][:k]
    live = np.flatnonzero(r >= floor * ref["beta0"])
    if live.size == 0:
        return 0.0, -1
    allowed = rtol * r[live] + 1e-15 * ref["beta0"] * r[live] / cb[live]
    ex = np.abs(h[live] - r[live]) / allowed
    if not np.all(np.isfinite(ex)):
        return np.inf, int(live[np.flatnonzero(~np.isfinite(ex))[0]])
    i = int(np.argmax(ex))
    return float(ex[i]), int(live[i])


# ---------------------------------------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------------------------------------
def disc_spectrum(m, rho_max=0.9, seed=0):
    rng = np.random.default_rng(seed)
    rho = rho_max * rng.uniform(0.0, 1.0, m) ** 0.25
    return 1.0 + rho * np.exp(1j * rng.uniform(0.0, 2 * np.pi, m))


def cluster_spectrum(m, spread=1e-3, seed=0):
    """eigenvalues within `spread` of 1: successive Krylov vectors are nearly parallel"""
    rng = np.random.default_rng(seed)
    return 1.0 + spread * (rng.standard_normal(m) + 1j * rng.standard_normal(m))


def random_rhs(m, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(m) + 1j * rng.standard_normal(m)


def group_map(N, m, p=None):
    """g(i) = (i p) mod m with p coprime to m (default: the first prime above m / phi, golden-ratio spread)"""
    if p is None:
        p = int(m / 1.618033988749895) | 1
        while math.gcd(p, m) != 1:
            p += 2
    assert math.gcd(p, m) == 1
    return ((np.arange(N, dtype=np.int64) * p) % m).astype(np.int64)


def group_counts(gmap, m):
    return np.bincount(gmap, minlength=m).astype(np.int64)


def expand(v, gmap):
    return np.asarray(v)[gmap]


def exhausted_problem(kind, seed=0):
    """(N, groups m or None, lambda per group, b per group, restart or None):
        "small-N<n>"  N = n <= restart (default restart min(20, N))
        "unit"        lambda = 1 and b = e_1 at N = 5: an exactly zero subdiagonal in double as well
        "identity"    lambda = 1 at N = 1025: the first step leaves nothing to orthogonalise
        "seven"       7 groups with 7 distinct lambda at restart 30: the Krylov space closes after 7 steps"""
    if kind.startswith("small-N"):
        n = int(kind[len("small-N"):])
        return n, None, disc_spectrum(n, 0.9, seed), random_rhs(n, seed + 1), None
    if kind == "unit":                  # lambda = 1, b = e_1: the first step leaves w == 0 EXACTLY (h = 1, acc = 1 + 0i)
        b = np.zeros(5, complex)
        b[0] = 1.0
        return 5, None, np.ones(5, complex), b, None
    if kind == "identity":
        return 1025, None, np.ones(1025, complex), random_rhs(1025, seed + 1), None
    if kind == "seven":
        return 7 * 4099, 7, disc_spectrum(7, 0.9, seed), random_rhs(7, seed + 1), 30
    raise ValueError(kind)
