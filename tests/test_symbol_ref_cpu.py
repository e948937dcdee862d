"""The extended-precision symbol reference (tests/symbol_ref.py, tests/golden/symbol_*.npz) checked on the CPU: the closed-form
limits of the oracle against limits that involve no closed form, the long-double reduction against the oracle's, a few
fixture entries against mpmath, and the double-precision yardsticks of tests/test_gpu_symbol.py, printed per case."""
import os

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import symbol_ref as sr

LARGEST_GOLDEN = 788 * 1024          # the largest file tests/golden/ held before these fixtures


def test_fixture_sizes_and_shell_gaps():
    for name in list(sr.GV2D_CASES) + list(sr.TRAP_CASES) + ["gv3d_16_k8pi"]:
        assert os.path.getsize(os.path.join(sr.GOLDEN, f"symbol_{name}.npz")) <= LARGEST_GOLDEN, name
    for name, c in sr.GV2D_CASES.items():
        fx = sr.load(name)
        gap = float(fx["gap"])
        assert (gap == 0.0) == (c["q_shell"] >= 0) and (gap == 0.0 or gap >= 1e-3), (name, gap)
        assert abs(gap - sr.shell_gap(fx["q"], c["n"] * c["h"], c["k"], c["q_shell"])) <= 1e-12
        assert np.all(np.isfinite(fx["g"])) and np.all(np.diff(fx["q"]) > 0)
    assert abs(float(sr.load("gv2d_n32_k10")["gap"]) - 0.0116) < 1e-4
    for name, c in sr.GV3D_CASES.items():
        jx, jy, jz = (sr.fft_index(4 * d) for d in c["dims"])
        qs = np.unique(jx[:, None, None] ** 2 + jy[None, :, None] ** 2 + jz[None, None, :] ** 2)
        gap = sr.shell_gap(qs, c["dims"][0] * c["h"], c["k"], c["q_shell"])
        print(f"{name}: shell gap {gap:.4f}")
        assert gap == 0.0 or gap >= 1e-3, (name, gap)


def test_oracle_limits_agree_with_independent_limits():
    # 2D, k = 20 pi on the shell q = 1600 of n = 32, box 1
    fx = sr.load("gv2d_n32_k20pi")
    k, box = float(fx["k"]), 1.0
    got = complex(o.gtruncated2d(1.5 * box, k, np.array([k]), patch_singular=True)[0])
    want = complex(fx["limit_indep"])
    print(f"2D limit: oracle {got}, independent {want}, rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-13 * abs(want)
    # ... and the fixture's own entry at the shell (mpmath's closed form)
    assert abs(complex(fx["g"][fx["q"] == 1600][0]) - want) <= 1e-13 * abs(want)
    # 3D, k = 8 pi on the shell q = 256 of n = 16, box 1
    fx = sr.load("gv3d_16_k8pi")
    k = float(fx["k"])
    want = complex(fx["limit_indep"])
    got = complex(o.gtruncated3d(1.8 * box, k, np.array([k]), patch_singular=True)[0])
    print(f"3D limit: oracle {got}, independent {want}, rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= 1e-13 * abs(want)
    kk = (2 * sr.PI / 4) * np.sqrt(sr.LD(256))
    assert abs(complex(sr.gv3d_limit_closed(sr.LD(18) / 10, kk)) - want) <= 1e-13 * abs(want)


def test_long_double_reduction_agrees_with_the_oracle():
    rng = np.random.default_rng(7)
    for dims in [(5, 4, 6), (8, 3)]:
        P = tuple(4 * d for d in dims)
        G = rng.standard_normal(P) + 1j * rng.standard_normal(P)            # FFT order
        want = o.reduce_symbol(np.fft.fftshift(G), dims)                       # (the oracle takes the centred symbol)
        got = sr.reduce_symbol(G.astype(sr.CLD), dims, tuple(2 * d for d in dims), window="oracle")
        assert got.dtype == sr.CLD
        assert sr.err(got, want) <= 1e-13
        # the windows of the device (plan_finish_reduce: "crop"; the 3D Greengard-Vico builders: "wrap"), on 2n and on a wider
        # working grid: other symbols, the same cropped convolution
        b = rng.standard_normal(int(np.prod(dims))) + 0j
        for Q in (tuple(2 * d for d in dims), tuple(2 * d + 4 for d in dims)):
            for window in ("crop", "wrap"):
                Gw = sr.reduce_symbol(G.astype(sr.CLD), dims, Q, window=window).astype(np.complex128)
                if Gw.shape == want.shape:
                    # on 2n "wrap" is the oracle's window; "crop" drops offset -n, which a random kernel fills
                    assert (sr.err(Gw, want) <= 1e-13) == (window == "wrap")
                assert sr.err(o.convolve_reduced(Gw, b, dims), o.convolve_reduced(want, b, dims)) <= 1e-13, (Q, window)


def test_3d_reduction_takes_either_limit():
    # the patched lattice points enter the reduction as the closed-form limit or as the independent one: the same symbol
    fx = sr.load("gv3d_16_k8pi")
    a = sr.gv3d_yardstick("gv3d_16_k8pi", (32, 32, 32))[0]
    b = sr.gv3d_yardstick("gv3d_16_k8pi", (32, 32, 32), limit=complex(fx["limit_indep"]))[0]
    assert sr.err(a, b) <= 1e-13


def test_fixture_entries_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    fx = sr.load("gv2d_strip_k1000")
    box, k = mp.mpf(1), mp.mpf(1000)
    L = mp.mpf(3) / 2 * box
    a = 1j * mp.pi / 2 * L * mp.hankel1(0, L * k)
    b = 1j * mp.pi / 2 * L * k * mp.hankel1(1, L * k)
    for t in (0, 1, len(fx["q"]) // 2, len(fx["q"]) - 1):
        s = 2 * mp.pi / (4 * box) * mp.sqrt(int(fx["q"][t]))
        want = complex((1 + a * (s * mp.besselj(1, L * s)) - b * mp.besselj(0, L * s)) / (s * s - k * k))
        assert abs(complex(fx["g"][t]) - want) <= 4e-16 * abs(want), t
    fx = sr.load("trap_offcentre")
    c = sr.TRAP_CASES["trap_offcentre"]
    h = mp.mpf(c["h"])
    for i, j in [(0, 0), (3, 17), (20, 24)]:
        xe = mp.mpf(c["x0"]) - mp.mpf(c["n"] - 1) / 2 * h + h * i
        ye = mp.mpf(c["y0"]) - mp.mpf(c["m"] - 1) / 2 * h + h * j
        want = complex(mp.hankel1(0, mp.mpf(c["k"]) * mp.sqrt(xe * xe + ye * ye)))
        assert abs(complex(fx["table"][i, j]) - want) <= 4e-16 * abs(want), (i, j)


def test_fixtures_regenerate_byte_for_byte(tmp_path, monkeypatch):
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_symbol_golden", os.path.join(sr.GOLDEN, "make_symbol_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    monkeypatch.setattr(gen, "HERE", str(tmp_path))
    gen.mp.mp.dps = 40
    gen.trap("trap_n21", sr.TRAP_CASES["trap_n21"])
    gen.gv3d("gv3d_16_k8pi", sr.GV3D_CASES["gv3d_16_k8pi"])
    gen.gv2d("gv2d_32x20_k10", sr.GV2D_CASES["gv2d_32x20_k10"])
    for name in ("trap_n21", "gv3d_16_k8pi", "gv2d_32x20_k10"):
        f = f"symbol_{name}.npz"
        assert open(tmp_path / f, "rb").read() == open(os.path.join(sr.GOLDEN, f), "rb").read(), name


# the pruned working grids of the 3D cases (lsfc_padded_length per axis); FORCE_ROCFFT works on 2n
WORKING_GRIDS = {"gv3d_16_k10": (32, 32, 32), "gv3d_16x24x40_k9": (32, 48, 80), "gv3d_16_k8pi": (32, 32, 32),
                 "gv3d_20_k9": (48, 48, 48), "gv3d_128x8x8_k30": (256, 32, 32)}


def test_double_precision_yardsticks():
    # e_double per case: what two independent double evaluations miss the reference by.  Rounding level, far below the ceiling.
    rows = [(name,) + sr.gv2d_yardstick(name)[1:] for name in sr.GV2D_CASES]
    rows += [(name,) + sr.trap_yardstick(name)[1:] for name in sr.TRAP_CASES]
    rows += [(name,) + sr.gv3d_yardstick(name, Q)[1:] for name, Q in WORKING_GRIDS.items()]
    for name, e, es, el in rows:
        print(f"{name}: e_double {e:.2e} (scipy {es:.2e}, libm {el:.2e})")
        assert 0 < e < sr.CEILING / sr.MARGIN, name
    # the unpatched shell case: the reference is NaN exactly at q == 1600, and so are both double evaluations (err() checks it)
    ref, e, _, _ = sr.gv2d_yardstick("gv2d_n32_k20pi", patched=False)
    assert np.count_nonzero(~np.isfinite(ref)) == 12 and 0 < e < sr.CEILING / sr.MARGIN
