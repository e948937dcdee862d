"""CPU tests of the BiCGStab(l) restatement (tests/bicgstabl_ref.py) that the GPU suite measures the device solver against:
it is BiCGSTAB at l = 1, it solves, and every problem of the GPU suite is well enough conditioned for a 1e-10 comparison."""
import numpy as np
import pytest

import bicgstabl_ref as br

LD = np.clongdouble


def _bicgstab_textbook(b, lam, steps):
    """van der Vorst's BiCGSTAB on diag(lam) x = lam b from x = 0 in long double, shadow residual = initial residual;
    returns the residual norm after every step"""
    lam, rhs = lam.astype(LD), (lam * b).astype(LD)
    x = np.zeros(b.size, dtype=LD)
    r = rhs.copy()
    rhat = r.copy()
    rho_old = alpha = omega = LD(1)
    v = np.zeros_like(r)
    p = np.zeros_like(r)
    out = []
    for _ in range(steps):
        rho = np.vdot(rhat, r)
        beta = (rho / rho_old) * (alpha / omega)
        p = r + beta * (p - omega * v)
        v = lam * p
        alpha = rho / np.vdot(rhat, v)
        s = r - alpha * v
        t = lam * s
        omega = np.vdot(t, s) / np.vdot(t, t)
        x = x + alpha * p + omega * s
        r = s - omega * t
        rho_old = rho
        out.append(np.sqrt(np.sum(r.real ** 2 + r.imag ** 2)))
    return np.array(out), x


@pytest.mark.parametrize("rho", [0.5, 0.7, 0.9])
def test_l1_is_textbook_bicgstab(rho):
    N = 1025
    lam, b = br.disc_spectrum(N, rho, seed=31), br.random_rhs(N, seed=32)
    ref = br.bicgstabl_ref(b, pl=lam, l=1, reltol=1e-10, max_mv_products=600)
    assert ref["converged"] and ref["iters"] > 10
    tb, x = _bicgstab_textbook(b, lam, ref["iters"])
    # the last cycle may leave through the G[0,0] <= tol^2 exit, which records the residual BEFORE the minimal-residual step
    # (and skips it): every entry before it is a BiCGSTAB residual, the last one is at most that of the BiCG half step
    dev = np.max(np.abs(tb[:-1] - ref["resnorm_ld"][:-1]) / ref["resnorm_ld"][:-1])
    assert dev < 1e-12, f"rho={rho}: residuals of BiCGStab(1) and BiCGSTAB differ by {float(dev):.2e}"
    last = ref["resnorm_ld"][-1]
    assert last <= ref["tol"] and (abs(tb[-1] - last) <= 1e-12 * last or tb[-1] < last)
    assert np.max(np.abs(x - ref["x"])) <= 1e-9 * np.max(np.abs(x))        # both solve to 1e-10


_CASES = br.gpu_cases()
_RESULTS = {}


def _condition(label):
    if label not in _RESULTS:
        _RESULTS[label] = br.input_condition(_CASES[label])
    return _RESULTS[label]


@pytest.mark.parametrize("label", sorted(_CASES))
def test_it_solves(label):
    # the preconditioned system diag(pl) x = diag(pl) b: its true residual against reltol * ||diag(pl) b|| (from x0 = 0 this
    # is the tolerance itself; 1e-6 relative for the drift of the recursive residual in long double); a run that the cap
    # stopped must say so instead
    kw = _CASES[label]
    ref = _condition(label)[3]
    if not ref["converged"]:
        assert ref["mvps"] >= kw["max_mv_products"] and ref["breakdown"] is None, label
        return
    c = np.ones(ref["x"].size) if kw.get("counts") is None else np.asarray(kw["counts"], dtype=np.float64)
    nrm = lambda w: float(np.sqrt(np.sum(c * np.abs(w.astype(np.complex128)) ** 2)))   # noqa: E731
    pl, b = kw["pl"].astype(LD), kw["b"].astype(LD)
    # (initially_zero with x0 != 0 solves for the increment: the residual of x - x0)
    x = ref["x"] - (np.asarray(kw["x0"]).astype(LD) if kw.get("initially_zero") else 0)
    assert nrm(pl * (b - x)) <= br.DEFAULT_RELTOL * nrm(pl * b) * (1 + 1e-6), label


@pytest.mark.parametrize("label", sorted(_CASES))
def test_input_condition(label):
    dev, xdev, same, _ = _condition(label)
    assert same, f"{label}: the double-precision run stops elsewhere"
    assert dev < 1e-11, f"{label}: history deviates by {dev:.2e} in double precision"
    assert xdev < 1e-12, f"{label}: x deviates by {xdev:.2e} in double precision"


@pytest.mark.parametrize("l", br.WIDE_L)
def test_wide_l_is_outside_the_condition_but_bounded(l):
    # l = 5 ... 8 on the larger-l problem: up to 3.5e-11, 5.2e-11, 1.3e-10, 4.4e-10 over three summation orders -- above the
    # 1e-11 of the input condition, so the GPU suite makes no history comparison for them (it checks that they solve)
    lam, b = br.large_l_problem()
    worst = 0.0
    for seed in (7, 8, 9):
        dev, xdev, same, ref = br.input_condition(dict(b=b, pl=lam, l=l, max_mv_products=br.MAX_MV), seed=seed)
        assert same and ref["converged"] and xdev < 1e-12
        worst = max(worst, dev)
    assert worst < 1e-9, f"l={l}: {worst:.2e}"


def test_exhausted_space_and_breakdown_rule():
    # N <= 3 with l = 2 (and a cap above the default of N products): the space is exhausted inside the first or second cycle; the restatement ends converged with a
    # finite x that solves the system
    for N in (1, 2, 3):
        lam, b = br.disc_spectrum(N, 0.9, seed=N), br.random_rhs(N, seed=N + 1)
        for dtype in (LD, np.complex128):
            ref = br.bicgstabl_ref(b, pl=lam, l=2, dtype=dtype, max_mv_products=20)
            assert ref["converged"] and np.all(np.isfinite(ref["x"])), (N, dtype)
            assert np.max(np.abs(lam * (ref["x"] - b))) <= 1e-8 * np.max(np.abs(lam * b)), (N, dtype)
    # b == 0: converged at once, no cycle
    ref = br.bicgstabl_ref(np.zeros(4, complex), pl=np.ones(4, complex), l=2)
    assert ref["converged"] and ref["iters"] == 0 and ref["mvps"] == 1
    # a shadow residual orthogonal to the residual: rho == 0 then sigma == 0 -- breakdown, x untouched and finite
    b = np.array([1.0, 0.0], complex)
    ref = br.bicgstabl_ref(b, pl=np.array([1.0, 2.0], complex), l=1, r_shadow=np.array([0.0, 1.0], complex))
    assert not ref["converged"] and ref["breakdown"] == "sigma" and np.all(ref["x"] == 0) and ref["iters"] == 1
