"""The reference of the off-grid sampling operator (tests/receivers_ref.py) pinned by identities; no device."""
import numpy as np
import pytest

import receivers_ref as ref

H, K = 1.0 / 8, 11.0
GRIDS = {3: ((6, 5, 4), (-0.37, -0.30, -0.21)), 2: ((7, 5), (-0.37, -0.30))}


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("kind", [0, 1])
def test_adjoint_identity(ndim, kind):
    # <w, R q> = <R^H w, q> to 1e-13
    dims, origin = GRIDS[ndim]
    rng = np.random.default_rng(5)
    coords = ref.random_directions(rng, 5, ndim) * (1.0 if kind else 2.5)
    R = ref.dense(kind, dims, origin, H, K, coords)
    q, w = ref.cvec(rng, R.shape[1]), ref.cvec(rng, R.shape[0])
    lhs, rhs = np.vdot(w, R @ q), np.vdot(R.conj().T @ w, q)
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)


@pytest.mark.parametrize("ndim", [2, 3])
def test_far_field_is_the_limit_of_the_point_rows(ndim):
    # R_points(rho theta) q -> e^{ik rho} / rho^((d-1)/2) R_far(theta) q; the error falls as 1/rho: 3.5e-5 (3D) and 4.5e-5 (2D)
    # at rho = 1e4 on these grids, a factor 20 inside the gate
    dims, origin = GRIDS[ndim]
    rng = np.random.default_rng(7)
    theta = ref.random_directions(rng, 5, ndim)
    rho = 1e4
    q = ref.cvec(rng, int(np.prod(dims)))
    near = ref.dense_points(dims, origin, H, K, rho * theta) @ q
    far = np.exp(1j * K * rho) / rho ** ((ndim - 1) / 2) * (ref.dense_far(dims, origin, H, K, theta) @ q)
    err = ref.rel(near, far)
    print(f"far-field limit, {ndim}D, rho = {rho:g}: relative l2 {err:.3e}")
    assert err <= 1e-3


def test_3d_row_is_the_formula_of_sampleG3D():
    # src/FastConvolution3D.jl:182-188 forms R = sqrt((X - xs)^2 + (Y - ys)^2 + (Z - zs)^2) on the mesh arrays and samples
    # exp(1im*k*R) ./ (4*pi*R); here with the weight h^d of the convolution kernel and an off-grid source
    dims, origin = GRIDS[3]
    x, y, z = (origin[a] + H * np.arange(dims[a]) for a in range(3))
    Xg, Yg, Zg = np.meshgrid(x, y, z, indexing="ij")
    X, Y, Z = (A.reshape(-1, order="F") for A in (Xg, Yg, Zg))
    p = np.array([0.113, -0.071, 0.402])
    Rd = np.sqrt((X - p[0]) ** 2 + (Y - p[1]) ** 2 + (Z - p[2]) ** 2)
    row = np.exp(1j * K * Rd) * H ** 3 / (4 * np.pi * Rd)
    assert ref.rel(ref.dense_points(dims, origin, H, K, p[None, :])[0], row) <= 1e-14


def test_grid_points_are_x_fastest():
    X = ref.grid_points((3, 2), (1.0, 10.0), 0.5)
    assert np.array_equal(X[:4], [[1.0, 10.0], [1.5, 10.0], [2.0, 10.0], [1.0, 10.5]])
