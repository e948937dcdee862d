"""Dense numpy reference of the Born operator's reciprocal mode (include/lsfc.h, "Reciprocal mode"), over tests/born_ref.py.  With the
receiver fields V = M^-1 R^T (row r: the field of receiver r used as a source) and R M^-T = V^T,

    (J dnu)[s, r] = -k^2 sum_i dnu[i] u_s[i] v_r[i]
    (J^H r)[i]    = -k^2 sum_s conj(u_s[i]) sum_r conj(v_r[i]) r[s, r]

and a numpy.longdouble statement of the two contractions of lsfc_born_contract for arbitrary U and V, with the sums of magnitudes
that the rounding bounds of tests/test_gpu_born_reciprocal.py are made of.  Test infrastructure, no GPU."""
import numpy as np

import born_ref as ref


def receiver_fields(G, R, nu, k):
    """V = (M^-1 R^T)^T: (nrecv, N)"""
    return np.linalg.solve(ref.dense_M(G, nu, k), R.T).T


def J(U, V, k, dnu):
    return -k * k * (U * dnu) @ V.T


def JH(U, V, k, r):
    return -k * k * (np.conj(U) * (r @ np.conj(V))).sum(axis=0)


def _ld(z):
    z = np.asarray(z)
    return z.real.astype(np.longdouble), (z.imag.astype(np.longdouble) if np.iscomplexobj(z) else np.zeros(z.shape, np.longdouble))


def _mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def contract_n_ld(U, V, x, scale):
    """out[s, r] = scale sum_i (x[i] u_s[i]) v_r[i] in long double -> (re, im, mag), mag[s, r] = |scale| sum_i |x||u_s||v_r|"""
    w = _mul(_ld(x), _ld(U))                                                     # (nsrc, N)
    v = _ld(V)
    t = w[0] @ v[0].T - w[1] @ v[1].T, w[0] @ v[1].T + w[1] @ v[0].T
    re, im = _mul(_ld(np.complex128(scale)), t)
    mag = abs(scale) * (np.abs(x)[None, :] * np.abs(U)) @ np.abs(V).T
    return re, im, mag


def contract_h_ld(U, V, x, scale, start=None):
    """out[i] = start[i] + conj(scale) sum_s conj(u_s[i]) sum_r conj(v_r[i]) x[s, r] in long double -> (re, im, mag),
    mag[i] = |scale| sum_{s, r} |u_s[i]||v_r[i]||x[s, r]|"""
    u, v, xr = _ld(U), _ld(V), _ld(x)
    vc = v[0], -v[1]
    q = xr[0] @ vc[0] - xr[1] @ vc[1], xr[0] @ vc[1] + xr[1] @ vc[0]              # (nsrc, N)
    t = _mul((u[0], -u[1]), q)
    re, im = _mul(_ld(np.conj(np.complex128(scale))), (t[0].sum(axis=0), t[1].sum(axis=0)))
    if start is not None:
        s = _ld(start)
        re, im = re + s[0], im + s[1]
    mag = abs(scale) * (np.abs(U) * (np.abs(x) @ np.abs(V))).sum(axis=0)
    return re, im, mag


def err_ld(got, re, im):
    """|got - (re + i im)| entry by entry, as doubles"""
    got = np.asarray(got)
    gi = got.imag if np.iscomplexobj(got) else np.zeros(got.shape)
    return np.hypot((got.real.astype(np.longdouble) - re).astype(float), (gi.astype(np.longdouble) - im).astype(float))
