"""The device symbol builders (csrc/symbol.hip) and the symbol storage (k_permute_symbol, plan_setup_symbol_rows) entry by entry.

Generators.  Each builder's symbol is read back through working_symbol() and compared with the extended-precision reference of
tests/symbol_ref.py in the metric e(v) = max|v - ref| / max|ref|.  The bound comes from the reference side only:
    e(device) <= MARGIN * e_double  and  e(device) < 1e-10,
e_double the larger error of two independent double evaluations of the same formula against the same reference (scipy's, and
libm's through ctypes), MARGIN = 8 the project's margin for two double computations of equal depth (where
the measured ratios are tabled).  Every case prints e(device), e_double and their ratio.
  2D Greengard-Vico, trapezoidal: flags = LITERAL, so the working symbol is the literal one (its FFT for the trapezoidal rule) / total.
  3D Greengard-Vico: FORCE_ROCFFT gives the natural-order reduced symbol on 2n; the pruned plans are decoded (below), built through
  the symbol's symmetry (default) and on the whole grid (LSFC_SYMBOL_FULL=1).  Both builders keep every offset of the working grid
  (symbol_ref.reduce_symbol, window "wrap").

Storage.  decode() turns working_symbol() of a pruned plan back into natural FFT order with lsfc_storage_order and the `store`
line of describe_passes(), following the layout documented above k_permute_symbol, undoes the 1/total scale and asserts that
every padding slot is exactly 0.  Plans built from a seeded random literal symbol on the 4n grid, symmetrised per axis, must
decode to the long-double reduction of that symbol within 1e-13, in the layout the case expects.
"""
import ctypes

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import symbol_ref as sr
from test_gpu_apply_forms import parse, symmetrise

pytestmark = pytest.mark.gpu
LITERAL, FORCE_ROCFFT, PATCH = 1, 2, 4
STORAGE_TOL = 1e-13
ENV = ("LSFC_SYM_EVEN_Y", "LSFC_SYM_EVEN_Z", "LSFC_2D_TILED", "LSFC_SYMBOL_FULL", "LSFC_POW2_ONLY")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def judge(what, dev, ref, e_double):
    e = sr.err(dev, ref)
    print(f"{what}: e(device) {e:.3e}  e_double {e_double:.3e}  ratio {e / e_double:.2f}")
    assert e < sr.CEILING, (what, e)
    assert e <= sr.MARGIN * e_double, (what, e, e_double, e / e_double)
    return e


# ---------------------------------------------------------------------------- decoding the stored symbol
def storage_order(lsfc, L):
    perm = (ctypes.c_int64 * L)()
    lsfc._lib.check(lsfc._lib.load().lsfc_storage_order(L, perm))
    perm = np.array(perm)
    assert sorted(perm) == list(range(L))
    return perm


def half_line(perm):
    """frequencies of the slots of a half-stored even line of L points: slots j < L/2 in storage order, slot L/2 = frequency L/2"""
    L = len(perm)
    assert np.all(perm[:L // 2] < L // 2)
    return np.concatenate([perm[:L // 2], [L // 2]])


def mirror_fill(G, axis):
    """the entries above L/2 along `axis` from their mirrors (an even line stores k <= L/2 only)"""
    L = G.shape[axis]
    idx = [slice(None)] * G.ndim
    src = list(idx)
    idx[axis], src[axis] = np.arange(L // 2 + 1, L), L - np.arange(L // 2 + 1, L)
    G[tuple(idx)] = G[tuple(src)]


def decode(lsfc, M):
    """working_symbol() of a pruned plan -> (the symbol in natural FFT order on the working grid, unscaled, index [kx, ky(, kz)];
    the parsed store line)"""
    desc = parse(M.describe_passes())
    assert desc["pipeline"] == "pruned-hip"
    st = desc["store"]
    Q = [int(v) for v in M.padded_dims]
    sym = M.working_symbol()
    px = storage_order(lsfc, Q[0]).reshape(Q[0] // 8, 8)
    if Q[2] > 1:
        Lx, Ly, Lz = Q
        py, pz = storage_order(lsfc, Ly), storage_order(lsfc, Lz)
        rows, hz = st["sym_rows"], st["sym_hz"]
        assert rows in (Ly, Ly // 2 + 1) and hz in (Lz, Lz // 2 + 8) and sym.size == Lx * rows * hz, (st, Q, sym.size)
        assert st["ytab"] == int(rows != Ly) and st["zmirror"] == int(hz != Lz) and st["tile2d"] == 0
        rowky = py if rows == Ly else py[py <= Ly // 2]             # the storage-ordered rows with ky <= Ly/2
        kz = pz if hz == Lz else half_line(pz)
        A = sym.reshape(Lx // 8, rows, hz, 8)                        # out[xi + 8*(j + hz*(row + rows*xb))]
        assert np.all(A[:, :, len(kz):, :] == 0), "padding slots of the half lines"
        G = np.full(Q, np.nan + 0j)
        G[px[:, None, None, :], rowky[None, :, None, None], kz[None, None, :, None]] = A[:, :, :len(kz), :]
        if hz != Lz:
            mirror_fill(G, 2)
        if rows != Ly:
            mirror_fill(G, 1)
    else:
        Lx, Ly = Q[:2]
        py = storage_order(lsfc, Ly)
        G = np.full((Lx, Ly), np.nan + 0j)
        if st["tile2d"]:
            hz = Ly // 2 + 8
            assert st["zmirror"] == 1 and st["sym_rows"] == 1 and st["sym_hz"] == hz and sym.size == Lx * hz
            ky = half_line(py)
            A = sym.reshape(Lx // 8, hz, 8)                          # the 3D layout, one row per tile, the line axis is y
            assert np.all(A[:, len(ky):, :] == 0), "padding slots of the half lines"
            G[px[:, None, :], ky[None, :, None]] = A[:, :len(ky), :]
        else:
            ky = half_line(py) if st["zmirror"] else py
            assert sym.size == Lx * len(ky)
            A = sym.reshape(len(ky), Lx)                             # out[sx + Lx*row]
            G[px.reshape(-1)[None, :], ky[:, None]] = A
        if st["zmirror"]:
            mirror_fill(G, 1)
    return G * float(np.prod(Q)), st


def natural(M):
    """working_symbol() of a rocFFT plan: natural order on the plan's grid, x fastest, scaled by 1 / total"""
    Q = [int(v) for v in M.padded_dims]
    Q = Q if Q[2] > 1 else Q[:2]
    with np.errstate(invalid="ignore"):                             # (an unpatched symbol holds Inf / NaN)
        return M.working_symbol().reshape(Q, order="F") * float(np.prod(Q))


def covered(G):
    assert not np.any(np.isnan(G)), "decode left entries unset"
    return G


# ---------------------------------------------------------------------------- generators: 2D Greengard-Vico
def build_gv2d(lsfc, name, flags):
    c = sr.GV2D_CASES[name]
    x, y = sr.grid_axis(c["n"], c["h"]), sr.grid_axis(c["m"], c["h"])
    M = lsfc.buildFastConvolution(x, y, c["h"], c["k"], o.gaussian_bump, quadRule="Greengard_Vico", flags=flags)
    assert M.pipeline == "rocfft-literal" and tuple(M.padded_dims) == (4 * c["n"], 4 * c["m"], 1)
    G = natural(M)
    M.close()
    return G


@pytest.mark.parametrize("name", ["gv2d_n32_k10", "gv2d_n33_k10", "gv2d_32x20_k10", "gv2d_strip_k1000"])
def test_gv2d_literal_symbol(lsfc, name):
    ref, e_double, _, _ = sr.gv2d_yardstick(name)
    judge(name, build_gv2d(lsfc, name, LITERAL), ref, e_double)


def test_gv2d_on_the_shell_patched(lsfc):
    name = "gv2d_n32_k20pi"
    fx = sr.load(name)
    ref, e_double, _, _ = sr.gv2d_yardstick(name)
    G = build_gv2d(lsfc, name, LITERAL | PATCH)
    judge(name + " patched", G, ref, e_double)
    # the twelve patched entries against the limit that involves no closed form
    _, q = sr.gv2d_literal(fx)
    shell = q == int(fx["q_shell"])
    assert np.count_nonzero(shell) == 12
    d = float(np.max(np.abs(G[shell] - complex(fx["limit_indep"]))) / np.max(np.abs(ref)))
    print(f"{name}: patched entries against the independent limit {d:.3e}")
    assert d <= sr.MARGIN * e_double


def test_gv2d_on_the_shell_unpatched(lsfc):
    name = "gv2d_n32_k20pi"
    ref, e_double, _, _ = sr.gv2d_yardstick(name, patched=False)
    G = build_gv2d(lsfc, name, LITERAL)
    _, q = sr.gv2d_literal(sr.load(name))
    assert np.array_equal(~np.isfinite(G), q == 1600)
    judge(name + " unpatched", G, ref, e_double)


# ---------------------------------------------------------------------------- generators: 2D trapezoidal
@pytest.mark.parametrize("name", sorted(sr.TRAP_CASES))
def test_trapezoidal_literal_symbol(lsfc, name):
    c = sr.TRAP_CASES[name]
    ref, e_double, _, _ = sr.trap_yardstick(name)
    x, y = c["x0"] + c["h"] * np.arange(c["n"]), c["y0"] + c["h"] * np.arange(c["m"])
    M = lsfc.buildFastConvolution(x, y, c["h"], c["k"], o.gaussian_bump, quadRule="trapezoidal", flags=LITERAL)
    assert M.pipeline == "rocfft-literal" and tuple(M.padded_dims) == (2 * c["n"] - 1, 2 * c["m"] - 1, 1)
    judge(name, natural(M), ref, e_double)
    M.close()


# ---------------------------------------------------------------------------- generators: 3D Greengard-Vico
def build_gv3d(lsfc, name, flags):
    c = sr.GV3D_CASES[name]
    ax = [sr.grid_axis(d, c["h"]) for d in c["dims"]]
    return lsfc.buildFastConvolution3D(*ax, None, None, None, c["h"], c["k"], np.zeros(int(np.prod(c["dims"]))), flags=flags)


@pytest.mark.parametrize("name", ["gv3d_16_k10", "gv3d_16x24x40_k9", "gv3d_16_k8pi"])
def test_gv3d_reduced_builder(lsfc, name):
    c = sr.GV3D_CASES[name]
    Q = tuple(2 * d for d in c["dims"])
    ref, e_double, _, _ = sr.gv3d_yardstick(name, Q)
    if c["q_shell"] >= 0:
        # the reference takes the patched lattice points from the closed form or from the independent limit: the same symbol
        other = sr.gv3d_yardstick(name, Q, limit=complex(sr.load(name)["limit_indep"]))[0]
        assert sr.err(other, ref) <= 1e-13
    M = build_gv3d(lsfc, name, FORCE_ROCFFT | (PATCH if c["q_shell"] >= 0 else 0))
    assert M.pipeline == "rocfft-reduced" and tuple(M.padded_dims) == Q
    judge(name + " reduced builder", natural(M), ref, e_double)
    M.close()


@pytest.mark.parametrize("name,Q", [("gv3d_16x24x40_k9", (32, 48, 80)), ("gv3d_20_k9", (48, 48, 48)), ("gv3d_128x8x8_k30", (256, 32, 32))])
def test_gv3d_on_the_pruned_grid(lsfc, name, Q, monkeypatch):
    ref, e_double, _, _ = sr.gv3d_yardstick(name, Q)
    got = {}
    for builder, full in (("quarter", None), ("full", "1")):
        if full:
            monkeypatch.setenv("LSFC_SYMBOL_FULL", full)
        M = build_gv3d(lsfc, name, 0)
        assert M.pipeline == "pruned-hip" and tuple(M.padded_dims) == Q
        G, st = decode(lsfc, M)
        M.close()
        # a radial symbol: both builders end in the y- and z-even quarter storage
        assert (st["sym_rows"], st["sym_hz"], st["ytab"], st["zmirror"]) == (Q[1] // 2 + 1, Q[2] // 2 + 8, 1, 1), (builder, st)
        got[builder] = covered(G)
        judge(f"{name} {builder} builder", G, ref, e_double)
    d = sr.err(got["quarter"], got["full"])
    print(f"{name}: quarter against full builder {d:.3e}  ratio {d / e_double:.2f}")
    assert d <= sr.MARGIN * e_double


# ---------------------------------------------------------------------------- storage
class Literal:
    """a seeded random symbol on the 4n grid, even along `axes`, as FastM / FastM3D take it, and its long-double reduction"""

    def __init__(self, dims, Q, axes, seed, G=None):
        self.dims, self.Q = dims, Q
        P = tuple(4 * d for d in dims)
        rng = np.random.default_rng(seed)
        self.G = symmetrise(rng.standard_normal(P) + 1j * rng.standard_normal(P), axes) if G is None else G       # FFT order
        self.nu = rng.uniform(-0.3, 0.3, int(np.prod(dims)))
        self.b = rng.standard_normal(self.nu.size) + 1j * rng.standard_normal(self.nu.size)
        self.ref = sr.reduce_symbol(self.G.astype(sr.CLD), dims, Q) if np.all(np.isfinite(self.G)) else None

    def plan(self, lsfc):
        P, d = self.G.shape, self.dims
        Gc = np.fft.fftshift(self.G)
        if len(d) == 3:
            M = lsfc.FastM3D(Gc, self.nu, *P, *d, 2.0)
        else:
            M = lsfc.FastM(Gc, self.nu, *P, *d, 2.0, quadRule="Greengard_Vico")
        assert M.pipeline == "pruned-hip" and tuple(M.padded_dims)[:len(d)] == tuple(self.Q)
        return M

    def check(self, lsfc, **store):
        M = self.plan(lsfc)
        G, st = decode(lsfc, M)
        M.close()
        assert {k: st[k] for k in store} == store, (st, store)
        e = sr.err(covered(G), self.ref)
        print(f"dims {self.dims} store {store}: decoded symbol against the long-double reduction {e:.3e}")
        assert e <= STORAGE_TOL
        return G


@pytest.mark.parametrize("axes,store", [
    ((), dict(sym_rows=48, sym_hz=80, ytab=0, zmirror=0)),
    ((1,), dict(sym_rows=25, sym_hz=80, ytab=1, zmirror=0)),
    ((2,), dict(sym_rows=48, sym_hz=48, ytab=0, zmirror=1)),
    ((1, 2), dict(sym_rows=25, sym_hz=48, ytab=1, zmirror=1)),
])
def test_storage_3d(lsfc, axes, store):
    Literal((16, 24, 40), (32, 48, 80), axes, seed=40 + len(axes) + sum(axes)).check(lsfc, **store)


def test_storage_3d_resampled_grid(lsfc):
    # 4n = 80 x 48 x 72 -> Q = 48 x 32 x 48, not 2n: the resample of plan_finish_reduce
    Literal((20, 12, 18), (48, 32, 48), (1, 2), seed=48).check(lsfc, sym_rows=17, sym_hz=32, ytab=1, zmirror=1)


@pytest.mark.parametrize("dims,Q,axes,tiled,store", [
    ((32, 16), (64, 32), (), None, dict(zmirror=0, tile2d=0)),
    ((32, 16), (64, 32), (0, 1), "0", dict(zmirror=1, tile2d=0)),
    ((32, 16), (64, 32), (0, 1), "1", dict(zmirror=1, tile2d=8 * 16, sym_rows=1, sym_hz=24)),
    ((40, 24), (80, 48), (0, 1), "1", dict(zmirror=1, tile2d=0)),          # 80 / 8 = 10 tiles, no whole groups of 8: rows
])
def test_storage_2d(lsfc, dims, Q, axes, tiled, store, monkeypatch):
    if tiled is not None:
        monkeypatch.setenv("LSFC_2D_TILED", tiled)
    Literal(dims, Q, axes, seed=sum(dims) + len(axes)).check(lsfc, **store)


def perturbed_literal(delta):
    """an even symbol whose REDUCED form is changed by delta * max|G2| at one entry of a y-mirror pair (and at its z mirror, so
    that the symbol stays z-even), carried back to the 4n grid: -> (Literal, the pair, max|G2|, e_double of the reduction)"""
    dims, Q = (16, 24, 40), (32, 48, 80)
    base = Literal(dims, Q, (1, 2), seed=77)
    G2 = base.ref.astype(np.complex128)
    top = float(np.abs(G2).max())
    a, b = (3, 5, 7), (3, Q[1] - 5, 7)
    G2[a] += delta * top
    G2[3, 5, Q[2] - 7] += delta * top
    # the literal of this reduced symbol: its kernel on Q, moved to the 4n grid offset by offset (all of Q: -Q/2 .. Q/2-1)
    T, P = np.fft.ifftn(G2), tuple(4 * d for d in dims)
    d = [np.arange(-(q // 2), q // 2) for q in Q]
    TP = np.zeros(P, dtype=np.complex128)
    TP[np.ix_(*(dd % p for dd, p in zip(d, P)))] = T[np.ix_(*(dd % q for dd, q in zip(d, Q)))]
    lit = Literal(dims, Q, (), seed=77, G=np.fft.fftn(TP))
    e_double = sr.err(sr.reduce_symbol(lit.G, dims, Q, fft=np.fft), lit.ref)
    return lit, a, b, top, e_double


def test_mirror_threshold_below(lsfc):
    # 1e-15 of the largest entry: even to the plan (threshold 1e-13), half storage; what decodes is the input within delta
    delta = 1e-15
    lit, a, b, top, e_double = perturbed_literal(delta)
    M = lit.plan(lsfc)
    G, st = decode(lsfc, M)
    M.close()
    assert (st["sym_rows"], st["ytab"], st["sym_hz"], st["zmirror"]) == (25, 1, 48, 1), st
    e = sr.err(covered(G), lit.ref)
    print(f"delta {delta:g}: decoded against the input {e:.3e}  (e_double of the reduction {e_double:.3e})")
    assert e <= STORAGE_TOL and e <= delta + sr.MARGIN * e_double


def test_mirror_threshold_above(lsfc):
    # 1e-11: not even in y, every row stored (the symbol stays z-even), and both entries of the pair come back as they are
    delta = 1e-11
    lit, a, b, top, _ = perturbed_literal(delta)
    M = lit.plan(lsfc)
    G, st = decode(lsfc, M)
    M.close()
    assert (st["sym_rows"], st["ytab"], st["sym_hz"], st["zmirror"]) == (48, 0, 48, 1), st
    assert sr.err(covered(G), lit.ref) <= STORAGE_TOL
    want = complex(lit.ref[a] - lit.ref[b])
    assert abs(want) > 0.8 * delta * top
    assert abs((G[a] - G[b]) - want) <= 1e-2 * abs(want)


def test_non_finite_symbol_is_stored_in_full(lsfc):
    # a NaN anywhere in the literal symbol makes every entry of the reduced one NaN: such a symbol is never "even"
    dims, Q = (16, 24, 40), (32, 48, 80)
    lit = Literal(dims, Q, (1, 2), seed=5)
    lit.G[3, 4, 5] = np.nan
    M = lit.plan(lsfc)
    st = parse(M.describe_passes())["store"]
    y = M * lit.b
    sym = M.working_symbol()
    M.close()
    assert (st["sym_rows"], st["ytab"], st["sym_hz"], st["zmirror"]) == (48, 0, 80, 0), st
    assert sym.size == 32 * 48 * 80 and np.all(np.isnan(sym))
    assert not np.any(np.isfinite(y))


def test_unpatched_shell_symbol_is_stored_in_full(lsfc):
    # the case the guard of pw_mirror_deviation names: omega on a lattice shell, unpatched, through the pruned 2D pipeline
    c = sr.GV2D_CASES["gv2d_n32_k20pi"]
    x = sr.grid_axis(c["n"], c["h"])
    M = lsfc.buildFastConvolution(x, x, c["h"], c["k"], o.gaussian_bump, quadRule="Greengard_Vico")
    assert M.pipeline == "pruned-hip" and tuple(M.padded_dims) == (64, 64, 1)
    st = parse(M.describe_passes())["store"]
    sym = M.working_symbol()
    y = M * o.random_vector(c["n"] ** 2)
    M.close()
    assert (st["zmirror"], st["tile2d"]) == (0, 0) and sym.size == 64 * 64 and np.all(np.isnan(sym)), st
    assert not np.any(np.isfinite(y))
    # ... and patched, the same plan stores the even half
    M = lsfc.buildFastConvolution(x, x, c["h"], c["k"], o.gaussian_bump, quadRule="Greengard_Vico", flags=PATCH)
    st = parse(M.describe_passes())["store"]
    M.close()
    assert st["zmirror"] == 1, st
