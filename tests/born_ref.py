"""Dense numpy reference of linearised scattering (include/lsfc.h, "linearised scattering"), written from the formulas and
independent of the kernels.  With M = I + k^2 G diag(nu), M u_s = u_inc_s and d_s = -k^2 R (nu .* u_s):

    J_s dnu = -k^2 R M^-T (u_s .* dnu)
    J^H r   = sum_s -k^2 conj(u_s .* p_s),   M p_s = R^T conj(r_s)

Dense G comes from the oracle's operator applied to identity columns (with nu = 1: (M - I) / k^2), dense R from
receivers_ref.dense, every solve is numpy.linalg.solve.  Test infrastructure, no GPU."""
import collections
import functools

import numpy as np

from oracle import lsfc_oracle as o
import receivers_ref as rref

POINTS, FAR = 0, 1
Case = collections.namedtuple("Case", "dims k amp")
# kh = 0.5, 0.8, 1.0 on the cubes (h = 1 / n), kh = 0.5 in 2D; the oracle's 3D builder takes even cubes, its 2D GV builder squares
CASES = {
    "6^3": Case((6, 6, 6), 3.0, 0.3),
    "8^3-kh0.8": Case((8, 8, 8), 6.4, 0.5),
    "8^3-kh1.0": Case((8, 8, 8), 8.0, 1.0),
    "10^2": Case((10, 10), 5.0, 0.3),
}


def axes_of(dims):
    """examples/example3D.jl: x = -a/2:h:a/2-h with h = 1 / n of the first axis, the same h on every axis"""
    h = 1.0 / dims[0]
    return [-0.5 + h * np.arange(v) for v in dims], h


def coords_of(dims):
    ax, _ = axes_of(dims)
    return o.grid2d(*ax) if len(dims) == 2 else o.grid3d(*ax)


def bump(amp, *X):
    """a Gaussian bump without a symmetry"""
    r2 = sum(x ** 2 for x in X)
    return amp * np.exp(-10.0 * r2) * (1.0 + 0.2 * X[0] - 0.1 * X[-1])


def nu_of(case, complex_=False):
    nu = bump(case.amp, *coords_of(case.dims))
    return nu * (1.0 + 0.3j) + 0.01j if complex_ else nu


def perturbation(case, seed=7, complex_=False):
    rng = np.random.default_rng(seed)
    N = int(np.prod(case.dims))
    d = rng.standard_normal(N)
    return d + 1j * rng.standard_normal(N) if complex_ else d


def oracle_operator(case, nu):
    ax, h = axes_of(case.dims)
    X = coords_of(case.dims)
    f = lambda *_: nu                                       # noqa: E731
    if len(case.dims) == 2:
        return o.build_fast_convolution(ax[0], ax[1], h, case.k, f, quadRule="Greengard_Vico")
    return o.build_fast_convolution3d(*ax, *X, h, case.k, f)


@functools.lru_cache(maxsize=None)
def dense_G(name):
    """the oracle's Green's matrix of a case, column by column: (M - I) e_i / k^2 with nu = 1; read only"""
    case = CASES[name]
    N = int(np.prod(case.dims))
    Mo = oracle_operator(case, np.ones(N))
    G = np.empty((N, N), dtype=np.complex128)
    e = np.zeros(N, dtype=np.complex128)
    for i in range(N):
        e[i] = 1.0
        G[:, i] = (o.mul(Mo, e) - e) / case.k ** 2
        e[i] = 0.0
    G.setflags(write=False)
    return G


def dense_M(G, nu, k):
    return np.eye(G.shape[0]) + k * k * G * np.asarray(nu)[None, :]


def receivers(case, kind, count, seed=5):
    """far-field directions, or point receivers on a sphere of 2.5 box sizes"""
    th = rref.random_directions(np.random.default_rng(seed), count, len(case.dims))
    return th if kind == FAR else 2.5 * th


def dense_R(case, kind, coords):
    ax, h = axes_of(case.dims)
    return rref.dense(kind, case.dims, tuple(a[0] for a in ax), h, case.k, coords)


def plane_waves(case, nsrc, seed=9):
    th = rref.random_directions(np.random.default_rng(seed), nsrc, len(case.dims))
    X = np.stack(coords_of(case.dims), axis=1)
    return np.exp(1j * case.k * (th @ X.T))                 # (nsrc, N)


def forward(G, R, nu, k, U_inc):
    """-> (U, d): the total fields (nsrc, N) and the data (nsrc, nrecv)"""
    U = np.linalg.solve(dense_M(G, nu, k), U_inc.T).T
    return U, -k * k * (U * nu) @ R.T


def J(G, R, nu, k, U, dnu):
    X = np.linalg.solve(dense_M(G, nu, k).T, (U * dnu).T)   # (N, nsrc)
    return -k * k * (R @ X).T


def JH(G, R, nu, k, U, r):
    P = np.linalg.solve(dense_M(G, nu, k), R.T @ np.conj(r).T)    # (N, nsrc)
    return (-k * k * np.conj(U * P.T)).sum(axis=0)


def dense_J(G, R, nu, k, U):
    """J as a (nsrc nrecv, N) matrix"""
    Minv_T = np.linalg.inv(dense_M(G, nu, k).T)
    return np.concatenate([-k * k * (R @ (Minv_T * U[s][None, :])) for s in range(U.shape[0])], axis=0)


def misfit(G, R, nu, k, U_inc, d_obs):
    U, d = forward(G, R, nu, k, U_inc)
    res = d - d_obs
    g = JH(G, R, nu, k, U, res)
    return 0.5 * float(np.vdot(res, res).real), (g if np.iscomplexobj(nu) else g.real)


rel, cvec = rref.rel, rref.cvec
