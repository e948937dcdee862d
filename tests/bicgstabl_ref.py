"""Test infrastructure for the device BiCGStab(l) (csrc/bicgstab.hip): a long-double restatement of its solve over a
diagonal operator and a diagonal left preconditioner, and the list of problems the GPU tests drive it with.

    bicgstabl_ref(b, a, pl, counts, l, max_mv_products, reltol, abstol, x0, initially_zero, r_shadow, dtype, perm)
        left-preconditioned BiCGStab(l) for  diag(pl) diag(a) x = diag(pl) b  with the control flow of lsfc_bicgstabl:
        init / initially_zero, the shadow residual (the preconditioned initial residual unless r_shadow is given), l BiCG
        steps, the Gram matrix, the exit G[0,0] <= tol^2, gamma by Gaussian elimination with partial pivoting in `dtype`,
        the minimal-residual update, one history entry per cycle (the norm of rs[0] computed from the vector), the
        `mvps < max_mv_products` test at the head of a cycle, and the breakdown rule (a rho, sigma or gamma that is zero
        where it divides, or not finite: the update is skipped, the residual of the last finite iterate decides).

        a / pl: per-group diagonals, or callables v -> A v, v -> Pl \\ v on full vectors (a real operator in complex128).
        Vectors are constant on GROUPS as in gmres_ref: group g stands for counts[g] equal entries.
        dtype = complex128 with perm (a permutation of the groups) is the same algorithm in plain double precision with
        another order of summation: the INPUT CONDITION of a problem is that this stays close to the long-double run.

        Returns a dict: resnorm, iters (cycles), mvps, converged, x (per group), beta0, tol, cycle_beta (beta0 for every
        entry, so that gmres_ref.history_excess applies), breakdown (None or the name of the scalar)."""
import math

import numpy as np

from gmres_ref import disc_spectrum, random_rhs, group_map, group_counts, history_excess  # noqa: F401

DEFAULT_RELTOL = math.sqrt(2.220446049250313e-16)


def _solve(M, y, dtype):
    """Gaussian elimination with partial pivoting in `dtype`; None if a pivot is zero or the solution is not finite"""
    M, y = M.astype(dtype).copy(), y.astype(dtype).copy()
    n = y.size
    for p in range(n):
        mag = M[p:, p].real ** 2 + M[p:, p].imag ** 2
        k = p + int(np.argmax(mag))
        if not (mag[k - p] > 0) or not np.isfinite(mag[k - p]):
            return None
        if k != p:
            M[[p, k]] = M[[k, p]]
            y[[p, k]] = y[[k, p]]
        for a in range(p + 1, n):
            f = M[a, p] / M[p, p]
            M[a, p + 1:] -= f * M[p, p + 1:]
            y[a] -= f * y[p]
    for a in range(n - 1, -1, -1):
        y[a] = (y[a] - np.sum(M[a, a + 1:] * y[a + 1:])) / M[a, a]
    return y if np.all(np.isfinite(y)) else None


def bicgstabl_ref(b, a=None, pl=None, counts=None, l=2, max_mv_products=None, reltol=None, abstol=0.0, x0=None,
                  initially_zero=False, r_shadow=None, dtype=np.clongdouble, perm=None):
    b = np.asarray(b).astype(dtype)
    m = b.size
    real = np.longdouble if dtype == np.clongdouble else np.float64
    c = np.ones(m, dtype=real) if counts is None else np.asarray(counts, dtype=np.float64).astype(real)
    N = int(m if counts is None else np.sum(counts))
    a = a if a is None or callable(a) else np.asarray(a).astype(dtype)
    pl = pl if pl is None or callable(pl) else np.asarray(pl).astype(dtype)
    maxmv = N if max_mv_products is None or max_mv_products <= 0 else int(max_mv_products)
    reltol = DEFAULT_RELTOL if reltol is None else reltol
    x = np.zeros(m, dtype=dtype) if x0 is None else np.asarray(x0).astype(dtype)
    order = np.arange(m) if perm is None else np.asarray(perm)

    dot = lambda u, w: np.sum((c * np.conj(u) * w)[order])                              # noqa: E731
    nrm2 = lambda w: np.sqrt(np.sum((c * (w.real * w.real + w.imag * w.imag))[order]))    # noqa: E731
    A = (lambda v: v.copy()) if a is None else a if callable(a) else (lambda v: a * v)  # noqa: E731
    P = (lambda v: v) if pl is None else pl if callable(pl) else (lambda v: pl * v)     # noqa: E731
    bad = lambda s, divides=False: (not np.isfinite(s)) or (divides and s == 0)         # noqa: E731

    rs = np.zeros((l + 1, m), dtype=dtype)
    us = np.zeros((l + 1, m), dtype=dtype)
    if initially_zero:
        rs[0], mvps = P(b.copy()), 0
    else:
        rs[0], mvps = P(b - A(x)), 1
    rt = rs[0].copy() if r_shadow is None else np.asarray(r_shadow).astype(dtype)
    sigma = dtype(1)
    beta0 = nrm2(rs[0])
    tol = max(reltol * float(beta0), abstol)
    current, converged, breakdown = beta0, bool(beta0 <= tol), None
    hist = []
    with np.errstate(all="ignore"):
        while not converged and breakdown is None and mvps < maxmv:
            sigma = -sigma
            for j in range(l):
                rho = dot(rt, rs[j])
                if breakdown is None and (bad(rho) or bad(sigma, True) or bad(rho / sigma)):
                    breakdown = "rho" if bad(rho) else "sigma"
                if breakdown is None:
                    beta = rho / sigma
                    us[:j + 1] = rs[:j + 1] - beta * us[:j + 1]
                us[j + 1] = P(A(us[j]))
                sigma_new = dot(rt, us[j + 1])
                if breakdown is None and (bad(sigma_new, True) or bad(rho / sigma_new)):
                    breakdown = "sigma"
                if breakdown is None:
                    sigma = sigma_new
                    alpha = rho / sigma
                    rs[:j + 1] -= alpha * us[1:j + 2]
                    x = x + alpha * us[0]
                rs[j + 1] = P(A(rs[j]))
                mvps += 2
            if breakdown is None:
                G = np.array([[dot(rs[i], rs[k]) for k in range(l + 1)] for i in range(l + 1)], dtype=dtype)
                if G[0, 0].real <= tol * tol:
                    current, converged = np.sqrt(G[0, 0].real), True
                    hist.append(current)
                    break
                gamma = _solve(G[1:, 1:], G[1:, 0], dtype)
                if gamma is None:
                    breakdown = "gamma"
            if breakdown is None:
                us[0] = us[0] - np.sum(gamma[:, None] * us[1:], axis=0)
                x = x + np.sum(gamma[:, None] * rs[:l], axis=0)
                rs[0] = rs[0] - np.sum(gamma[:, None] * rs[1:], axis=0)
                sigma = sigma * gamma[l - 1]
            current = nrm2(rs[0])
            if not np.isfinite(current):
                breakdown = breakdown or "residual"
            hist.append(current)
            converged = bool(current <= tol)
    n = len(hist)
    return {"resnorm": np.array(hist, dtype=np.float64), "resnorm_ld": np.array(hist), "iters": n, "mvps": mvps,
            "converged": converged, "x": x, "beta0": float(beta0), "tol": tol, "cycle_beta": np.full(n, float(beta0)),
            "breakdown": None if converged else breakdown}


# ---------------------------------------------------------------------------------------------------------------------
# the problems of tests/test_gpu_bicgstabl.py; tests/test_bicgstabl_ref_cpu.py checks the input condition of every one
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = [5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4095, 65538]
LARGE_L = [3, 4]        # l = 5 ... 8 break the input condition on this problem (3.5e-11 ... 4.4e-10 against 1e-11): the
WIDE_L = [5, 6, 7, 8]   # largest l that keeps it is 4; the wider ones get no history comparison on the GPU (they must solve)
GROUPED = [(1 << 20) + 3, (1 << 22) + 1]
GROUPS = 331
MAX_MV = 600            # of the length cases: enough for convergence at rho = 0.9 ...
SHORT_MV = 40           # ... but N = 63, 64, 65 would need more products than the space has dimensions: the last cycles
#                         before exhaustion break the input condition (up to 3.5e-7), so these stop at 40 products


def length_cap(N):
    return SHORT_MV if N in (63, 64, 65) else MAX_MV


def length_problem(N):
    """(lambda, b) of the vector-length cases, l in {1, 2}, rho = 0.9"""
    return disc_spectrum(N, 0.9, seed=N), random_rhs(N, seed=N + 1)


def large_l_problem():
    """(lambda, b) of the larger-l cases: N = 1025, rho = 0.5"""
    return disc_spectrum(1025, 0.5, seed=1025), random_rhs(1025, seed=1026)


def grouped_problem():
    """(lambda, b) per group of the large grouped cases: 331 groups, rho = 0.7, l = 2"""
    return disc_spectrum(GROUPS, 0.7, seed=3), random_rhs(GROUPS, seed=4)


def option_problem():
    """N = 1025, rho = 0.7: (lambda, b, x0, r_shadow) of the option cases (r_shadow, initially_zero, the cap)"""
    N = 1025
    return disc_spectrum(N, 0.7, seed=21), random_rhs(N, seed=22), 0.1 * random_rhs(N, seed=23), random_rhs(N, seed=24)


def input_condition(kw, seed=7):
    """(history deviation on entries >= 1e-9 beta0, x deviation, counts equal) of the plain complex128 run with a permuted
    summation order against the long-double run of the same problem"""
    ref = bicgstabl_ref(**kw)
    d = bicgstabl_ref(dtype=np.complex128, perm=np.random.default_rng(seed).permutation(np.asarray(kw["b"]).size), **kw)
    r, h = ref["resnorm"], d["resnorm"]
    k = min(r.size, h.size)
    live = np.flatnonzero(r[:k] >= 1e-9 * ref["beta0"])
    dev = float(np.max(np.abs(h[live] - r[live]) / r[live])) if live.size else 0.0
    c = np.ones(ref["x"].size) if kw.get("counts") is None else np.asarray(kw["counts"], dtype=np.float64)
    dx = (d["x"] - ref["x"]).astype(np.complex128)
    xdev = float(np.sqrt(np.sum(c * np.abs(dx) ** 2) / np.sum(c * np.abs(ref["x"].astype(np.complex128)) ** 2)))
    same = (d["iters"], d["mvps"], d["converged"]) == (ref["iters"], ref["mvps"], ref["converged"])
    return dev, xdev, same, ref


def gpu_cases():
    """label -> keyword arguments of bicgstabl_ref for every history comparison of the GPU suite"""
    cases = {}
    for N in LENGTHS:
        lam, b = length_problem(N)
        for l in (1, 2):
            cases[f"len-N{N}-l{l}"] = dict(b=b, pl=lam, l=l, max_mv_products=length_cap(N))
    lam, b = large_l_problem()
    for l in LARGE_L:
        cases[f"large-l{l}"] = dict(b=b, pl=lam, l=l, max_mv_products=MAX_MV)
    lam, b = grouped_problem()
    for N in GROUPED:
        cases[f"grouped-N{N}"] = dict(b=b, pl=lam, l=2, max_mv_products=MAX_MV, counts=group_counts(group_map(N, GROUPS), GROUPS))
    lam, b, x0, shadow = option_problem()
    cases["shadow"] = dict(b=b, pl=lam, l=2, r_shadow=shadow)
    cases["x0"] = dict(b=b, pl=lam, l=2, x0=x0)
    cases["x0-initially-zero"] = dict(b=b, pl=lam, l=2, x0=x0, initially_zero=True)
    cases["cap"] = dict(b=b, pl=lam, l=2, max_mv_products=14)
    return cases
