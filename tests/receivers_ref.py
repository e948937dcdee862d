"""numpy / scipy reference of the off-grid sampling operator R (include/lsfc.h, "off-grid sources and receivers"): the dense
nrecv x N matrix, formed entry by entry from the formulas of the header.  Written independently of the kernels: positions come
from index arithmetic on whole arrays, the 2D kernel from scipy's hankel1, the far-field rows from one exp of theta . x."""
import numpy as np
from scipy.special import hankel1


def grid_points(dims, origin, h):
    """(N, ndim) positions origin + h (ix, iy[, iz]), x fastest"""
    idx = np.indices(tuple(dims)[::-1])[::-1]                   # idx[a] has shape dims reversed: the last array axis is x
    return np.stack([np.asarray(origin[a]) + h * idx[a].reshape(-1).astype(np.float64) for a in range(len(dims))], axis=1)


def far_constant(ndim, k):
    """c_d: R_far = c_d h^d exp(-ik theta . x)"""
    return 1.0 / (4.0 * np.pi) if ndim == 3 else np.exp(0.25j * np.pi) / np.sqrt(8.0 * np.pi * k)


def dense_points(dims, origin, h, k, points):
    X = grid_points(dims, origin, h)
    P = np.asarray(points, dtype=np.float64).reshape(-1, len(dims))
    r = np.sqrt(((P[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    if len(dims) == 3:
        return h ** 3 * np.exp(1j * k * r) / (4.0 * np.pi * r)
    return h ** 2 * 0.25j * hankel1(0, k * r)


def dense_far(dims, origin, h, k, directions):
    X = grid_points(dims, origin, h)
    Th = np.asarray(directions, dtype=np.float64).reshape(-1, len(dims))
    return far_constant(len(dims), k) * h ** len(dims) * np.exp(-1j * k * (Th @ X.T))


def dense(kind, dims, origin, h, k, coords):
    return dense_points(dims, origin, h, k, coords) if kind == 0 else dense_far(dims, origin, h, k, coords)


def random_directions(rng, count, ndim):
    v = rng.standard_normal((count, ndim))
    return v / np.linalg.norm(v, axis=1)[:, None]


def cvec(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def rel(a, b):
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
