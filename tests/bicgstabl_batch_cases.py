"""The problems of the lock-step batch tests (tests/test_gpu_bicgstabl_batch.py), built from tests/bicgstabl_ref.py;
tests/test_bicgstabl_batch_cases_cpu.py checks the input condition of every member that is compared with the long-double
restatement, and pins the cycle counts the GPU test relies on.

A member is a dict of keyword arguments of bicgstabl_ref (b, pl, l, abstol, x0, r_shadow, max_mv_products, ...)."""
import numpy as np

import bicgstabl_ref as br

LEAVE_N = 1025
# cycles of the six members of leave_members(l): they leave the group at different cycles, one runs no cycle at all
LEAVE_CYCLES = {1: (14, 14, 15, 5, 2, 0), 2: (7, 7, 8, 3, 1, 0)}


def leave_abstol():
    lam, b = br.option_problem()[:2]
    return 1e-5 * float(np.linalg.norm(lam * b))


def leave_members(l):
    """six members on the option problem (N = 1025, rho = 0.7) with one shared abstol = 1e-5 ||lam b||: b; b from a
    non-zero x0; another right-hand side b2; 1e-3 b2 (the shared abstol is a much looser relative tolerance for it); a b
    with three non-zero entries (the Krylov space is exhausted); b = 0 (converged before the first cycle)"""
    lam, b, x0, _ = br.option_problem()
    b2 = br.random_rhs(LEAVE_N, seed=41)
    b3 = np.zeros(LEAVE_N, complex)
    b3[:3] = b[:3]
    common = dict(pl=lam, l=l, abstol=leave_abstol())
    return [dict(b=b, **common), dict(b=b, x0=x0, **common), dict(b=b2, **common), dict(b=1e-3 * b2, **common),
            dict(b=b3, **common), dict(b=np.zeros(LEAVE_N, complex), **common)]


def length_members(N, l, count=3):
    """`count` right-hand sides on the vector-length problem of bicgstabl_ref.length_problem(N)"""
    lam = br.length_problem(N)[0]
    return [dict(b=br.random_rhs(N, seed=100 + j), pl=lam, l=l, max_mv_products=br.length_cap(N)) for j in range(count)]


def breakdown_members():
    """N = 2, lam = (1, 2), l = 1, cap 10: member 0 breaks down in cycle 1 (sigma == 0, the problem of
    test_breakdown_keeps_the_last_finite_iterate), member 1 converges beside it"""
    lam = np.array([1.0, 2.0], complex)
    common = dict(pl=lam, l=1, max_mv_products=10)
    return [dict(b=np.array([1.0, 0.0], complex), r_shadow=np.array([0.0, 1.0], complex), x0=np.array([0.25, 0.0], complex), **common),
            dict(b=np.array([1.0, 1.0], complex), r_shadow=np.array([1.0, 2.0], complex), x0=np.zeros(2, complex), **common)]


def stack(members, key, N):
    """(nrhs, N) array of the members' `key` (zeros where a member has none)"""
    return np.array([np.zeros(N, complex) if m.get(key) is None else np.asarray(m[key], dtype=complex) for m in members])
