"""Pins the reciprocal-mode formulas (tests/born_reciprocal_ref.py) on the CPU: with V = M^-1 R^T the two contractions are J and J^H
of tests/born_ref.py at 1e-12, and exactly adjoint to each other; the long-double statement of the contractions agrees with the
double one.  Passes with or without the product's Born operator."""
import numpy as np
import pytest

import born_ref as ref
import born_reciprocal_ref as rr

NSRC, NRECV = 5, 9


@pytest.mark.parametrize("kind", [ref.FAR, ref.POINTS])
@pytest.mark.parametrize("complex_nu", [False, True])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_contractions_are_j_and_jh(name, complex_nu, kind):
    case = ref.CASES[name]
    G, k = ref.dense_G(name), case.k
    nu = ref.nu_of(case, complex_nu)
    R = ref.dense_R(case, kind, ref.receivers(case, kind, NRECV))
    U, _ = ref.forward(G, R, nu, k, ref.plane_waves(case, NSRC))
    V = rr.receiver_fields(G, R, nu, k)
    assert V.shape == (NRECV, G.shape[0])
    r = ref.cvec(np.random.default_rng(13), NSRC, NRECV)
    g = rr.JH(U, V, k, r)
    e_h = ref.rel(g, ref.JH(G, R, nu, k, U, r))
    worst = 0.0
    for complex_dnu in (False, True):
        dnu = ref.perturbation(case, complex_=complex_dnu)
        Jd = rr.J(U, V, k, dnu)
        e_j = ref.rel(Jd, ref.J(G, R, nu, k, U, dnu))
        dot = abs(np.vdot(r, Jd) - np.vdot(g, dnu)) / (np.linalg.norm(r) * np.linalg.norm(Jd))
        worst = max(worst, e_j, dot)
        print(f"  {name} complex nu {complex_nu} kind {kind} complex dnu {complex_dnu}: J {e_j:.1e}, JH {e_h:.1e}, dot {dot:.1e}")
        assert e_j <= 1e-12 and dot <= 1e-12, (e_j, dot)
    assert e_h <= 1e-12, e_h


def test_the_long_double_contractions_state_the_same_sums():
    rng = np.random.default_rng(3)
    N, nsrc, nrecv = 50, 3, 4
    U, V = ref.cvec(rng, nsrc, N), ref.cvec(rng, nrecv, N)
    scale = complex(-2.25, 0.75)
    for x in (rng.standard_normal(N), ref.cvec(rng, N)):
        re, im, mag = rr.contract_n_ld(U, V, x, scale)
        want = scale * (U * x) @ V.T
        assert rr.err_ld(want, re, im).max() <= 1e-13 * mag.max() and mag.shape == (nsrc, nrecv)
    x = ref.cvec(rng, nsrc, nrecv)
    start = ref.cvec(rng, N)
    re, im, mag = rr.contract_h_ld(U, V, x, scale, start)
    want = start + np.conj(scale) * (np.conj(U) * (x @ np.conj(V))).sum(axis=0)
    assert rr.err_ld(want, re, im).max() <= 1e-13 * mag.max() and mag.shape == (N,)
    # the two are adjoint for any scale: <y, N x> = <H y, x>
    xin = ref.cvec(rng, N)
    re, im, _ = rr.contract_n_ld(U, V, xin, scale)
    out_n = (re + 1j * im).astype(complex)
    re, im, _ = rr.contract_h_ld(U, V, x, scale)
    out_h = (re + 1j * im).astype(complex)
    assert abs(np.vdot(x, out_n) - np.vdot(out_h, xin)) <= 1e-13 * np.linalg.norm(x) * np.linalg.norm(out_n)
