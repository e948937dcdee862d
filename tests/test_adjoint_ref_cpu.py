"""The yardstick of the transposed / adjoint operator tests (tests/adjoint_ref.py) against dense matrices: A is built column by
column from ``o.mul`` on three tiny grids, and want_T / want_H must be A.T / A.conj().T applied.  Also: G itself is symmetric
(what makes I + omega^2 diag(nu) G the transpose).  Bound 1e-13; rounding of a dozen flops per entry, ~2e-16, was observed."""
import numpy as np
import pytest

from oracle import lsfc_oracle as o
import adjoint_ref as ar


def _grid(n, inclusive):
    h = 1.0 / (n - 1) if inclusive else 1.0 / n
    return -0.5 + h * np.arange(n), h


def _operators():
    x, h = _grid(8, False)
    yield "2d-gv-8", o.build_fast_convolution(x, x, h, 6.0, o.gaussian_bump, quadRule="Greengard_Vico")
    x, h = _grid(7, True)
    yield "2d-trap-7", o.build_fast_convolution(x, x, h, 1.0 / h, o.gaussian_bump, quadRule="trapezoidal")
    x, h = _grid(4, False)
    z = x[:3]
    X, Y, Z = o.grid3d(x, x, z)
    yield "3d-gv-4x4x3", o.build_fast_convolution3d(x, x, z, X, Y, Z, h, 5.0, o.gaussian_bump)


OPS = dict(_operators())


def _dense(f, N):
    A = np.empty((N, N), dtype=np.complex128)
    for j in range(N):
        e = np.zeros(N, dtype=np.complex128)
        e[j] = 1.0
        A[:, j] = f(e)
    return A


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name", sorted(OPS))
def test_reference_is_the_dense_transpose_and_adjoint(name):
    Mo = OPS[name]
    N = int(np.asarray(Mo.nu).size)
    A = _dense(lambda v: o.mul(Mo, v), N)
    ref = ar.ref_of_oracle(Mo)
    rng = np.random.default_rng(11)
    for _ in range(3):
        y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        eT, eH = _rel(ref.T(y), A.T @ y), _rel(ref.H(y), A.conj().T @ y)
        print(f"{name}: T {eT:.2e}  H {eH:.2e}")
        assert eT < 1e-13 and eH < 1e-13
    # ... and the forward operator of the same pieces is A (the pieces are the right ones)
    y = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    assert _rel(y + Mo.omega ** 2 * ref.conv(np.asarray(Mo.nu).reshape(-1) * y), A @ y) < 1e-13


@pytest.mark.parametrize("name", sorted(OPS))
def test_green_matrix_is_symmetric(name):
    Mo = OPS[name]
    N = int(np.asarray(Mo.nu).size)
    G = _dense(ar.conv_of_oracle(Mo), N)
    d = float(np.linalg.norm(G - G.T) / np.linalg.norm(G))
    print(f"{name}: |G - G^T| / |G| = {d:.2e}")
    assert d < 1e-13


def test_adjoint_is_the_conjugated_transpose_of_the_conjugate():
    Mo = OPS["2d-gv-8"]
    ref = ar.ref_of_oracle(Mo)
    rng = np.random.default_rng(5)
    y = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    assert np.array_equal(ref.H(y), np.conj(ref.T(np.conj(y))))
    assert np.array_equal(ref.of("T")(y), ref.T(y))
