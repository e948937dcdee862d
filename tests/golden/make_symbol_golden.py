"""Writes tests/golden/symbol_*.npz: the reference values of tests/symbol_ref.py that need mpmath (40 digits), per case

  2D Greengard-Vico   n, m, h, k, q_shell, q (the distinct i^2 + j^2 of the 4n x 4m lattice), g (Gtruncated2D per q,
                      rounded to double; at q_shell the closed-form limit), gap (min |s^2 - k^2| / k^2 over the lattice);
                      on a shell also limit_indep
  2D trapezoidal      n, m, h, k, x0, y0 and q, g = H0^(1)(k h sqrt(q)) per distinct q > 0 of a centred grid (g = 0 at
                      q = 0, which D0 replaces), or table = H0^(1)(k r) on the whole (2n-1) x (2m-1) grid otherwise
  3D on a shell       limit_indep only (the 3D symbol itself is evaluated in long double at test time)

limit_indep: the unpatched formula at s = k (1 +- 1e-20) with 60 digits, averaged -- no closed form of the limit involved.
Every case asserts gap == 0 (on a shell) or gap >= 1e-3: nearer than that the formula itself is ill-conditioned.
The files carry fixed timestamps: a second run writes the same bytes.        python tests/golden/make_symbol_golden.py
"""
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import symbol_ref as sr               # noqa: E402


def save(name, **arrays):
    path = os.path.join(HERE, f"symbol_{name}.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
    print(f"{path}: {os.path.getsize(path)} bytes")


def gap_of(qs, box, k, q_shell):
    if q_shell >= 0:
        assert q_shell in qs
        return 0.0
    qk = (mp.mpf(k) * 4 * mp.mpf(box) / (2 * mp.pi)) ** 2
    gap = float(min(abs(int(q) - qk) for q in qs) / qk)
    assert gap >= 1e-3, gap
    return gap


def lattice_k(box, k, q_shell):
    """k as the reference takes it: the double, or on a shell the lattice value that the double rounds"""
    if q_shell < 0:
        return mp.mpf(k)
    kk = 2 * mp.pi / (4 * mp.mpf(box)) * mp.sqrt(q_shell)
    assert abs(kk - mp.mpf(k)) < 4e-16 * kk
    return kk


def averaged(f, k):
    mp.mp.dps = 60
    v = (f(k * (1 + mp.mpf(10) ** -20)) + f(k * (1 - mp.mpf(10) ** -20))) / 2
    mp.mp.dps = 40
    return complex(v)


def gv2d(name, c):
    n, m, q_shell = c["n"], c["m"], c["q_shell"]
    box = mp.mpf(n * c["h"])
    Lp, L = 4 * box, mp.mpf(3) / 2 * box
    k = lattice_k(box, c["k"], q_shell)
    i, j = sr.fft_index(4 * n), sr.fft_index(4 * m)
    qs = np.unique(i[:, None] ** 2 + j[None, :] ** 2)

    def g_of(s, k=k):
        a = 1j * mp.pi / 2 * L * mp.hankel1(0, L * k)
        b = 1j * mp.pi / 2 * L * k * mp.hankel1(1, L * k)
        return (1 + a * (s * mp.besselj(1, L * s)) - b * mp.besselj(0, L * s)) / (s * s - k * k)

    a = 1j * mp.pi / 2 * L * mp.hankel1(0, L * k)
    b = 1j * mp.pi / 2 * L * k * mp.hankel1(1, L * k)
    g = np.empty(len(qs), dtype=np.complex128)
    for t, q in enumerate(qs):
        if q == q_shell:
            g[t] = complex((a * L * k * mp.besselj(0, L * k) + b * L * mp.besselj(1, L * k)) / (2 * k))
        else:
            s = 2 * mp.pi / Lp * mp.sqrt(int(q))
            g[t] = complex((1 + a * (s * mp.besselj(1, L * s)) - b * mp.besselj(0, L * s)) / (s * s - k * k))
    out = dict(n=n, m=m, h=c["h"], k=c["k"], q_shell=q_shell, q=qs.astype(np.int64), g=g, gap=gap_of(qs, box, c["k"], q_shell))
    if q_shell >= 0:
        out["limit_indep"] = averaged(g_of, k)
    save(name, **out)


def trap(name, c):
    n, m, h, k = c["n"], c["m"], mp.mpf(c["h"]), mp.mpf(c["k"])
    out = dict(n=n, m=m, h=c["h"], k=c["k"], x0=c["x0"], y0=c["y0"])
    xe0, ye0 = mp.mpf(c["x0"]) - mp.mpf(n - 1) / 2 * h, mp.mpf(c["y0"]) - mp.mpf(m - 1) / 2 * h
    if abs(xe0 + (n - 1) * h) + abs(ye0 + (m - 1) * h) <= 1e-12 * h:       # centred (h = 1/20 is not a double: to rounding): r = h sqrt(q)
        i, j = np.arange(2 * n - 1) - (n - 1), np.arange(2 * m - 1) - (m - 1)
        qs = np.unique(i[:, None] ** 2 + j[None, :] ** 2)
        out["q"] = qs.astype(np.int64)
        out["g"] = np.array([complex(mp.hankel1(0, k * h * mp.sqrt(int(q)))) if q else 0j for q in qs])
    else:
        out["table"] = np.array([[complex(mp.hankel1(0, k * mp.sqrt((xe0 + h * i) ** 2 + (ye0 + h * j) ** 2)))
                                  for j in range(2 * m - 1)] for i in range(2 * n - 1)])
    save(name, **out)


def gv3d(name, c):
    dims, q_shell = c["dims"], c["q_shell"]
    box = mp.mpf(dims[0] * c["h"])
    jx, jy, jz = (sr.fft_index(4 * d) for d in dims)
    qs = np.unique(jx[:, None, None] ** 2 + jy[None, :, None] ** 2 + jz[None, None, :] ** 2)
    gap = gap_of(qs, box, c["k"], q_shell)
    if q_shell < 0:
        return
    L, k = mp.mpf(18) / 10 * box, lattice_k(box, c["k"], q_shell)

    def g_of(s):
        return (-1 + mp.expj(L * k) * (mp.cos(L * s) - 1j * k * L * mp.sin(L * s) / (L * s))) / (k * k - s * s)

    save(name, dims=np.array(dims), h=c["h"], k=c["k"], q_shell=q_shell, gap=gap, limit_indep=averaged(g_of, k))


def main():
    mp.mp.dps = 40
    for name, c in sr.GV2D_CASES.items():
        gv2d(name, c)
    for name, c in sr.TRAP_CASES.items():
        trap(name, c)
    for name, c in sr.GV3D_CASES.items():
        gv3d(name, c)


if __name__ == "__main__":
    main()
