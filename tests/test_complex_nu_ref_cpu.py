"""The yardstick of the complex-nu tests (tests/complex_nu_ref.py) against dense matrices: A is built column by column from the
reference's forward apply, and N / T / H of the reference must be A, A.T and A.conj().T applied.  Bound 1e-13 relative
Frobenius (a dozen flops per entry; <= 1.2e-16 was observed).  Also: a real nu handed over as complex gives tests/adjoint_ref.py,
and Msp = As + k^2 AG diag(nu) of the sparsifying restatement's own pieces."""
import numpy as np
import pytest

from oracle import lsfc_oracle as o
import adjoint_ref as ar
import cases
import complex_nu_ref as cr
import sparsify_ref as sr


def _symmetrise(G, axes):
    for ax in axes:
        G = 0.5 * (G + np.roll(np.flip(G, axis=ax), 1, axis=ax))
    return G


def complex_nu(rng, N):
    """real part U(-0.3, 0.3), imaginary part U(-0.2, 0.2), independent and of both signs"""
    return rng.uniform(-0.3, 0.3, N) + 1j * rng.uniform(-0.2, 0.2, N)


def _reduced(dims, grid, seed):
    rng = np.random.default_rng(seed)
    G2 = _symmetrise(rng.standard_normal(grid) + 1j * rng.standard_normal(grid), tuple(range(len(grid))))
    N = int(np.prod(dims))
    nu = complex_nu(rng, N)
    return cr.ref_of_reduced(G2, dims, nu, 2.0), ar.Ref(ar.conv_of_reduced(G2, dims), nu.real, 2.0), N


def _trap21():
    Mo = cases.case_2d("trap21")["M"]
    N = Mo.n * Mo.m
    nu = complex_nu(np.random.default_rng(21), N)
    return cr.ref_of_oracle(Mo, nu), ar.ref_of_oracle(Mo), N


CASES = {
    "reduced-4x3x5": lambda: _reduced((4, 3, 5), (8, 8, 16), 1),
    "reduced-6x5": lambda: _reduced((6, 5), (12, 10), 2),
    "trap21": _trap21,
}


def _dense(f, N):
    A = np.empty((N, N), dtype=np.complex128)
    for j in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[j] = 1.0
        A[:, j] = f(e)
    return A


def _fro(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_the_dense_operator_its_transpose_and_its_adjoint(name):
    ref, _, N = CASES[name]()
    assert np.iscomplexobj(ref.nu) and np.abs(ref.nu.imag).max() > 0.1
    A = _dense(ref.N, N)
    G = _dense(ref.conv, N)
    # A really is I + omega^2 G diag(nu) with the complex nu, and G is symmetric
    assert _fro(A, np.eye(N) + ref.omega ** 2 * G * ref.nu[None, :]) < 1e-13
    assert _fro(G, G.T) < 1e-13
    eT, eH = _fro(_dense(ref.T, N), A.T), _fro(_dense(ref.H, N), A.conj().T)
    print(f"{name}: T {eT:.2e}  H {eH:.2e}")
    assert eT < 1e-13 and eH < 1e-13
    # ... and on vectors: want_H(b) = conj(want_T(conj b)) exactly
    rng = np.random.default_rng(11)
    y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    assert np.array_equal(ref.H(y), np.conj(ref.T(np.conj(y))))
    assert _fro(ref.H(y), A.conj().T @ y) < 1e-13 and _fro(ref.T(y), A.T @ y) < 1e-13 and _fro(ref.N(y), A @ y) < 1e-13
    # the adjoint multiplies by conj(nu): with nu itself it is off at first order
    wrong = y + ref.omega ** 2 * ref.nu * np.conj(ref.conv(np.conj(y)))
    assert _fro(wrong, A.conj().T @ y) > 1e-3


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_real_nu_passed_as_complex_is_the_real_reference(name):
    ref, real_ref, N = CASES[name]()
    as_complex = cr.Ref(None, ref.conv, real_ref.nu.astype(np.complex128), ref.omega)
    rng = np.random.default_rng(12)
    y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    assert _fro(as_complex.T(y), real_ref.T(y)) < 1e-15 and _fro(as_complex.H(y), real_ref.H(y)) < 1e-15


def test_msp_ref_is_as_plus_k2_ag_diag_nu():
    n, k = 9, 7.0
    x, h = cases.grid(n, True)
    Mo = o.build_fast_convolution(x, x, h, k, o.gaussian_bump, quadRule="Greengard_Vico")
    rng = np.random.default_rng(13)
    nu_re = rng.uniform(-0.3, 0.3, n * n)
    built = sr.build(sr.conv_rows(Mo), n, n, nu=nu_re, k=k)
    # a real nu as complex: the restatement's own Msp
    M0 = cr.msp_ref(built, nu_re.astype(np.complex128), k)
    assert abs(M0 - built["Msp"]).max() <= 1e-15 * abs(built["Msp"]).max()
    # a complex nu: dense As + k^2 AG diag(nu), entry by entry
    nu = nu_re + 1j * rng.uniform(-0.2, 0.2, n * n)
    M1 = cr.msp_ref(built, nu, k).toarray()
    want = built["As"].toarray() + k ** 2 * built["AG"].toarray() * nu[None, :]
    assert np.abs(M1 - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(M1 - M0.toarray()).max() > 1e-3 * np.abs(want).max()
