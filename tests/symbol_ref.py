"""Extended-precision reference of the Fourier symbols that csrc/symbol.hip generates, entry by entry.  CPU only.

  3D Greengard-Vico   evaluated here in np.longdouble (64-bit mantissa) on the exact lattice s = (2 pi / Lp) sqrt(q),
                      q = jx^2 + jy^2 + jz^2 an integer, and reduced to a working grid Q with scipy.fft on clongdouble.
  2D Greengard-Vico,  Bessel / Hankel values from mpmath at 40 digits, far too slow for test time: they are read from the
  2D trapezoidal      fixtures tests/golden/symbol_*.npz that tests/golden/make_symbol_golden.py writes (one value per
                      distinct q = i^2 + j^2, rounded to double; the whole table for a grid that is not centred).

A case whose omega sits on a lattice shell, s == k at q == q_shell, is evaluated with k := (2 pi / Lp) sqrt(q_shell) in
extended precision (the double k of the test is that number rounded) and takes the limit there.

The yardstick of a generator test, e_double, is the larger error of two independent DOUBLE evaluations of the same formula
against the same reference, in the metric e(v) = max|v - ref| / max|ref|: the oracle's (scipy.special, scipy.fft) and one
through libm's j0 / j1 / y0 / y1 / cos / sin, called by ctypes, with numpy's FFT -- "another math library".
"""
import ctypes
import ctypes.util
import os

import numpy as np
import scipy.fft as sfft

from oracle import lsfc_oracle as o

LD, CLD = np.longdouble, np.clongdouble
PI = LD("3.14159265358979323846264338327950288419716939937510")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 8.0                 # two double computations of equal depth
CEILING = 1e-10

# name -> parameters.  box = n h of the x axis, a power of two times a small integer, so that Lp = 4 box and L are exact.
GV2D_CASES = {
    "gv2d_n32_k10":    dict(n=32, m=32, h=1 / 32, k=10.0, q_shell=-1),
    "gv2d_n33_k10":    dict(n=33, m=33, h=1 / 32, k=10.0, q_shell=-1),
    "gv2d_32x20_k10":  dict(n=32, m=20, h=1 / 32, k=10.0, q_shell=-1),
    "gv2d_strip_k1000": dict(n=1024, m=2, h=1 / 1024, k=1000.0, q_shell=-1),
    "gv2d_n32_k20pi":  dict(n=32, m=32, h=1 / 32, k=20 * np.pi, q_shell=1600),
}
TRAP_CASES = {
    "trap_n21":      dict(n=21, m=21, h=1 / 20, k=20.0, x0=-0.5, y0=-0.5),           # the parameters of cases.py "trap21"
    "trap_21x33":    dict(n=21, m=33, h=1 / 20, k=20.0, x0=-0.5, y0=-0.8),
    "trap_offcentre": dict(n=11, m=13, h=1 / 20, k=20.0, x0=0.125, y0=-0.4375),      # not centred at the origin
}
GV3D_CASES = {
    "gv3d_16_k10":      dict(dims=(16, 16, 16), h=1 / 16, k=10.0, q_shell=-1),
    "gv3d_16x24x40_k9": dict(dims=(16, 24, 40), h=1 / 16, k=9.0, q_shell=-1),
    "gv3d_16_k8pi":     dict(dims=(16, 16, 16), h=1 / 16, k=8 * np.pi, q_shell=256),
    "gv3d_20_k9":       dict(dims=(20, 20, 20), h=1 / 16, k=9.0, q_shell=-1),
    # (box 1/2: at box 1 the lattice point q = 365 lies 6.6e-4 from the shell of k = 30, inside the ill-conditioned band)
    "gv3d_128x8x8_k30": dict(dims=(128, 8, 8), h=1 / 256, k=30.0, q_shell=-1),
}


def err(v, ref):
    """e(v) = max|v - ref| / max|ref|; non-finite entries must coincide and are left out"""
    v, ref = np.asarray(v), np.asarray(ref)
    bad = ~np.isfinite(ref)
    assert np.array_equal(bad, ~np.isfinite(v)), "non-finite entries differ"
    d = np.abs((v.astype(CLD) - ref.astype(CLD))[~bad])
    return float(d.max() / np.abs(ref[~bad]).max())


def grid_axis(n, h):
    return -0.5 + h * np.arange(n)


def fft_index(P):
    """signed frequency index of every slot of an FFT-order axis of P points, the way symbol.hip counts: j < P/2 ? j : j - P"""
    j = np.arange(P)
    return np.where(j < P // 2, j, j - P)


def shell_gap(qs, box, k, q_shell):
    """min |s^2 - k^2| / k^2 over the lattice (q > 0 or not): exactly 0 for a case on a shell"""
    if q_shell >= 0:
        assert q_shell in qs
        return 0.0
    qk = (LD(k) * 4 * LD(box) / (2 * PI)) ** 2
    return float(np.min(np.abs(np.asarray(qs).astype(LD) - qk)) / qk)


# ---------------------------------------------------------------------------- 3D Greengard-Vico, long double
def gv3d_limit_closed(L, k):
    """(i L - (i/k) sin(Lk) e^{iLk}) / (2k), the limit of Gtruncated3D at s == k"""
    e = np.cos(L * k) + 1j * np.sin(L * k)
    return (1j * L - (1j / k) * np.sin(L * k) * e) / (2 * k)


def gv3d_of_s(L, k, s):
    """(-1 + e^{iLk} (cos(Ls) - i k L sin(Ls)/(Ls))) / (k^2 - s^2) in the precision of s; s == 0 takes sinc = 1"""
    s = np.asarray(s)
    Ls = L * s
    with np.errstate(divide="ignore", invalid="ignore"):
        snc = np.where(Ls == 0, LD(1), np.sin(Ls) / Ls)
        e = np.cos(L * k) + 1j * np.sin(L * k)
        return (-1 + e * (np.cos(Ls) - 1j * k * L * snc)) / (k * k - s * s)


def gv3d_literal(dims, box, k, q_shell=-1, limit=None):
    """literal symbol of buildFastConvolution3D on the (4n, 4m, 4l) lattice in FFT order, clongdouble, index [jx, jy, jz]"""
    box = LD(box)
    Lp, L = 4 * box, LD(18) / 10 * box
    jx, jy, jz = (fft_index(4 * d).astype(np.int64) for d in dims)
    q = jx[:, None, None] ** 2 + jy[None, :, None] ** 2 + jz[None, None, :] ** 2
    qs, inv = np.unique(q, return_inverse=True)
    kk = (2 * PI / Lp) * np.sqrt(LD(q_shell)) if q_shell >= 0 else LD(k)
    g = gv3d_of_s(L, kk, (2 * PI / Lp) * np.sqrt(qs.astype(LD))).astype(CLD)
    if q_shell >= 0:
        g[qs == q_shell] = gv3d_limit_closed(L, kk) if limit is None else limit
    return g[inv.reshape(q.shape)]


def gv3d_literal_double(dims, box, k, patch, libm):
    """the same symbol in double: the oracle's gtruncated3d, or the formula through libm's cos / sin (sinc as sin(Ls)/(Ls))"""
    Lp, L = 4 * box, 1.8 * box
    ax = [(2 * np.pi / Lp) * fft_index(4 * d).astype(np.float64) for d in dims]
    S = np.sqrt(ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2)
    if not libm:
        return o.gtruncated3d(L, float(k), S, patch)
    su, inv = np.unique(S, return_inverse=True)
    c, s = _libm_map("cos", L * su), _libm_map("sin", L * su)
    with np.errstate(divide="ignore", invalid="ignore"):
        snc = np.where(su == 0, 1.0, s / (L * su))
        e = complex(_libm()["cos"](L * k), _libm()["sin"](L * k))
        g = (-1 + e * (c - 1j * k * L * snc)) / (k * k - su * su)
    if patch:
        g = np.where(su == k, (1j * L - (1j / k) * _libm()["sin"](L * k) * e) / (2 * k), g)
    return g[inv.reshape(S.shape)]


# ---------------------------------------------------------------------------- the reduction onto a working grid
def reduce_symbol(G, dims, Q, origin=None, window="crop", fft=sfft):
    """G2 = fft_Q(resample(ifft_P(G))): G in FFT order on the literal grid P = G.shape (any precision), the kernel offset d
    at index (d + origin) mod P; the offsets of `window` are kept on the working grid Q, at index d mod Q, everything else
    is zero.  The cropped convolution reads the offsets -(n-1) .. n-1 only, so every window that holds them gives the same
    operator and another symbol:
      "crop"    -(n-1) .. n-1: plan_finish_reduce (pw_resample_kernel), the symbols handed over on a literal grid
      "wrap"    -Q/2 .. Q/2-1, all that Q holds: the Greengard-Vico builders symbol_gv3d_reduced (k_crop_xy_planes, k_crop_z)
                and symbol_gv3d_quarter (whose +Q/2 is the even kernel's -Q/2)
      "oracle"  -n .. n-1: the oracle's reduce_symbol on Q = 2n"""
    T = fft.ifftn(G)
    origin = origin or (0,) * len(dims)
    idx_src, idx_dst = [], []
    for n, P, Qa, og in zip(dims, G.shape, Q, origin):
        d = {"crop": np.arange(-(n - 1), n), "wrap": np.arange(-(Qa // 2), Qa - Qa // 2), "oracle": np.arange(-n, n)}[window]
        assert len(d) <= min(P, Qa) and d[0] <= -(n - 1) and d[-1] >= n - 1
        idx_src.append((d + og) % P)
        idx_dst.append(d % Qa)
    T2 = np.zeros(Q, dtype=T.dtype)
    T2[np.ix_(*idx_dst)] = T[np.ix_(*idx_src)]
    return fft.fftn(T2)


# ---------------------------------------------------------------------------- libm by ctypes
_LIBM = {}


def _libm():
    if not _LIBM:
        lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        for name in ("j0", "j1", "y0", "y1", "cos", "sin"):
            f = getattr(lib, name)
            f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
            _LIBM[name] = f
    return _LIBM


def _libm_map(name, x):
    f = _libm()[name]
    x = np.asarray(x, dtype=np.float64)
    return np.fromiter((f(v) for v in x.ravel()), dtype=np.float64, count=x.size).reshape(x.shape)


# ---------------------------------------------------------------------------- 2D Greengard-Vico from a fixture
def load(name):
    with np.load(os.path.join(GOLDEN, f"symbol_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def _lookup(fx, q):
    pos = np.searchsorted(fx["q"], q)
    assert np.array_equal(fx["q"][pos], q)
    return fx["g"][pos]


def gv2d_literal(fx, patched=True):
    """literal symbol of buildFastConvolution (4n x 4m) in FFT order, index [i, j]; the shell entries are the limit, or NaN"""
    i, j = fft_index(4 * int(fx["n"])), fft_index(4 * int(fx["m"]))
    q = i[:, None] ** 2 + j[None, :] ** 2
    g = _lookup(fx, q)
    if not patched and int(fx["q_shell"]) >= 0:
        g = np.where(q == int(fx["q_shell"]), np.nan + 1j * np.nan, g)
    return g, q


def gv2d_literal_double(n, m, box, k, patch, libm):
    """the same symbol in double, FFT order: the oracle's gtruncated2d (scipy.special), or the formula through libm"""
    Lp, L = 4 * box, 1.5 * box
    kx, ky = ((2 * np.pi / Lp) * fft_index(4 * d).astype(np.float64) for d in (n, m))
    S = np.sqrt(kx[:, None] ** 2 + ky[None, :] ** 2)
    if not libm:
        return o.gtruncated2d(L, float(k), S, patch)
    f = _libm()
    a = 1j * np.pi / 2 * L * complex(f["j0"](L * k), f["y0"](L * k))
    b = 1j * np.pi / 2 * L * k * complex(f["j1"](L * k), f["y1"](L * k))
    su, inv = np.unique(S, return_inverse=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (1 + a * (su * _libm_map("j1", L * su)) - b * _libm_map("j0", L * su)) / (su ** 2 - k ** 2)
    if patch:
        g = np.where(su == k, (a * L * k * f["j0"](L * k) + b * L * f["j1"](L * k)) / (2 * k), g)
    return g[inv.reshape(S.shape)]


# ---------------------------------------------------------------------------- 2D trapezoidal from a fixture
def trap_d0(k, h):
    _, D = o.reference_vals_trap_rule()
    return D[int(round(k * h)) - 1]


def trap_ge(fx):
    """Ge of buildGConv, (2n-1) x (2m-1), index [i, j], from the fixture's Hankel values (the centre entry is D0)"""
    n, m, h = int(fx["n"]), int(fx["m"]), float(fx["h"])
    if "table" in fx:
        H = fx["table"].copy()
    else:
        i, j = np.arange(2 * n - 1) - (n - 1), np.arange(2 * m - 1) - (m - 1)
        H = _lookup(fx, i[:, None] ** 2 + j[None, :] ** 2)
    H[n - 1, m - 1] = trap_d0(float(fx["k"]), h)
    return (0.25j * LD(h) * LD(h)) * H.astype(CLD)


def trap_ge_double(n, m, h, k, x0, y0, libm):
    x, y = x0 + h * np.arange(n), y0 + h * np.arange(m)
    D0 = trap_d0(k, h)
    if not libm:
        return o.build_gconv(x, y, h, n, m, D0, k)
    xe = x[0] - (n - 1) / 2 * h + h * np.arange(2 * n - 1)
    ye = y[0] - (m - 1) / 2 * h + h * np.arange(2 * m - 1)
    R = np.sqrt(xe[:, None] ** 2 + ye[None, :] ** 2)
    R[n - 1, m - 1] = 1.0
    Ge = 0.25j * (_libm_map("j0", k * R) + 1j * _libm_map("y0", k * R)) * h ** 2
    Ge[n - 1, m - 1] = 0.25j * D0 * h ** 2
    return Ge


# ---------------------------------------------------------------------------- the yardsticks, one per case
def yardstick(ref, scipy_value, libm_value):
    es, el = err(scipy_value, ref), err(libm_value, ref)
    return max(es, el), es, el


def gv2d_yardstick(name, patched=True):
    c, fx = GV2D_CASES[name], load(name)
    ref, _ = gv2d_literal(fx, patched)
    box = c["n"] * c["h"]
    return (ref,) + yardstick(ref, *(gv2d_literal_double(c["n"], c["m"], box, c["k"], patched, lm) for lm in (False, True)))


def trap_yardstick(name):
    c, fx = TRAP_CASES[name], load(name)
    ref = sfft.fftn(trap_ge(fx))
    dbl = [trap_ge_double(c["n"], c["m"], c["h"], c["k"], c["x0"], c["y0"], lm) for lm in (False, True)]
    return (ref,) + yardstick(ref, sfft.fftn(dbl[0]), np.fft.fftn(dbl[1]))


def gv3d_yardstick(name, Q, limit=None):
    """reference and double evaluations of the reduced symbol of a 3D case on the working grid Q, as the builders window it"""
    c = GV3D_CASES[name]
    dims, box, patch = c["dims"], c["dims"][0] * c["h"], c["q_shell"] >= 0
    ref = reduce_symbol(gv3d_literal(dims, box, c["k"], c["q_shell"], limit), dims, Q, window="wrap")
    dbl = [reduce_symbol(gv3d_literal_double(dims, box, c["k"], patch, lm), dims, Q, window="wrap", fft=np.fft if lm else sfft)
           for lm in (False, True)]
    return (ref,) + yardstick(ref, *dbl)
