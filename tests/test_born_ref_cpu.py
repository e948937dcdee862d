"""Pins the dense reference of linearised scattering (tests/born_ref.py) on the CPU: J against central differences of the forward
map, the dot identity between J and J^H, and the conditioning that makes the 1e-10 parity bound of tests/test_gpu_born.py one the
reference itself supports.  Passes with or without the product's Born operator."""
import numpy as np
import pytest

import born_ref as ref

EPS = 1e-5


def setup(name, complex_nu):
    case = ref.CASES[name]
    G = ref.dense_G(name)
    nu = ref.nu_of(case, complex_nu)
    R = ref.dense_R(case, ref.FAR, ref.receivers(case, ref.FAR, 5))
    U_inc = ref.plane_waves(case, 3)
    return case, G, nu, R, U_inc


@pytest.mark.parametrize("complex_nu", [False, True])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_j_against_central_differences_and_the_dot_identity(name, complex_nu):
    case, G, nu, R, U_inc = setup(name, complex_nu)
    k = case.k
    cond = np.linalg.cond(ref.dense_M(G, nu, k))
    assert cond <= 10.0, cond
    assert np.abs(G - G.T).max() <= 1e-14 * np.abs(G).max()
    U, d = ref.forward(G, R, nu, k, U_inc)
    dnu = ref.perturbation(case, complex_=complex_nu)
    Jd = ref.J(G, R, nu, k, U, dnu)
    fd = (ref.forward(G, R, nu + EPS * dnu, k, U_inc)[1] - ref.forward(G, R, nu - EPS * dnu, k, U_inc)[1]) / (2 * EPS)
    err = ref.rel(Jd, fd)
    print(f"  {name} complex nu {complex_nu}: cond(M) {cond:.2f}, J vs central difference {err:.2e}")
    assert err <= 1e-8, err
    # <r, J dnu> = <J^H r, dnu>
    rng = np.random.default_rng(13)
    r = ref.cvec(rng, *Jd.shape)
    lhs, rhs = np.vdot(r, Jd), np.vdot(ref.JH(G, R, nu, k, U, r), dnu)
    assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(r) * np.linalg.norm(Jd), abs(lhs - rhs)
    # the matrix form agrees with the two applies
    Jm = ref.dense_J(G, R, nu, k, U)
    assert ref.rel(Jm @ dnu, Jd.reshape(-1)) <= 1e-12
    assert ref.rel(Jm.conj().T @ r.reshape(-1), ref.JH(G, R, nu, k, U, r)) <= 1e-12


def test_gradient_of_the_misfit_for_a_real_nu():
    # phi(nu + t dnu) - phi(nu - t dnu) = 2 t <grad, dnu> + O(t^3) with grad = Re J^H (d - d_obs)
    case, G, nu, R, U_inc = setup("6^3", False)
    d_obs = ref.forward(G, R, 1.3 * nu, case.k, U_inc)[1]
    phi, grad = ref.misfit(G, R, nu, case.k, U_inc, d_obs)
    assert grad.dtype == np.float64 and phi > 0
    dnu = ref.perturbation(case)
    t = 1e-5
    fd = (ref.misfit(G, R, nu + t * dnu, case.k, U_inc, d_obs)[0] - ref.misfit(G, R, nu - t * dnu, case.k, U_inc, d_obs)[0]) / (2 * t)
    assert abs(fd - grad @ dnu) <= 1e-7 * abs(fd), (fd, grad @ dnu)
