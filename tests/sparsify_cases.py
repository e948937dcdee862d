"""The grids on which the sparsifying assembly (csrc/sparsify.hip, lsfc_sparsify_build) is compared with the restatement of
the reference (tests/sparsify_ref.py), shared by tests/test_sparsify_cases_cpu.py and tests/test_gpu_sparsify_shapes.py (test
infrastructure, not product code; no GPU).

k_gram and k_refine walk the N columns of G in tiles of GCOLS = 64 with at most GPARTS = 256 workgroups per class, so a
workgroup takes a second tile only from N = 16385 on; the 2D class tables mix n and m; the smallest grids are one partial
tile.  Every entry of CASES sits on one of those edges (`why`, and DESIGN.md "Sparsifying matrices").  nu has no symmetry, so
a row-for-column or x-for-y slip in the stamping moves Msp.

`reference(case)` runs the restatement once per process and keeps, next to what sparsify_ref.build returns, per class

    refine[c] = (e(corrected), e(uncorrected), b_c)    gram_refine of the class's rows against the SVD vector; b_c below
    row0[c]                                            the reference's row of the class's first sample source

b_c = eps * sigma_max / (sigma_-2 - sigma_min) is the first-order perturbation bound of the smallest left singular vector
under a backward error of eps * sigma_max: the accuracy of the SVD reference itself."""
import collections
import functools

import numpy as np

from oracle import lsfc_oracle as o
import sparsify_ref as ref

EPS = float(np.finfo(np.float64).eps)
# The device bound (tests/test_gpu_sparsify_shapes.py): 4 x the largest e(corrected) / b_c of gram_refine over CASES, which is
# 0.681 at trap-21x41 (tests/test_sparsify_cases_cpu.py asserts that CASES stays under MARGIN / 4).  The factor 4 covers the
# device's summation order (64-column tiles, FMA, 256 partials) against numpy's.  Measured against the emulation, never
# against the device.
MARGIN = 2.73
GCOLS, GPARTS = 64, 256                                    # csrc/sparsify.hip

Case = collections.namedtuple("Case", "kind dims k why")   # k None: 1 / h, as the example drivers choose it

# kind "trap":  2D trapezoidal through buildFastConvolution(x, y, ...), rows sparsify_ref.direct_rows
#      "lowk":  2D trapezoidal with the caller's D0 through buildSparseA / buildSparseAG (no round(k h) limit): As, AG only
#      "gv2":   2D Greengard-Vico, square, rows sparsify_ref.conv_rows
#      "gv3":   3D Greengard-Vico, even axes, rows sparsify_ref.gv3d_rows
CASES = [
    Case("trap", (5, 5), None, "smallest 2D grid: one partial tile, 25 live columns of 64"),
    Case("trap", (5, 7), None, "smallest, n < m"),
    Case("trap", (7, 5), None, "smallest, n > m"),
    Case("trap", (9, 5), None, "smallest, n > m, N = 45"),
    Case("trap", (21, 41), None, "rectangular, n < m"),
    Case("trap", (41, 21), None, "rectangular, n > m"),
    Case("trap", (127, 129), None, "N = 16383: exactly 256 chunks, last tile 63 columns, one tile per workgroup"),
    Case("trap", (129, 127), None, "the same, n > m"),
    Case("trap", (129, 129), None, "N = 16641: 261 chunks, five workgroups take two tiles, last tile one live column"),
    Case("trap", (257, 65), None, "N = 16705: 262 chunks, strongly rectangular"),
    Case("trap", (183, 181), None, "N = 33123: 518 chunks, every workgroup two tiles, six take three"),
    Case("lowk", (41, 41), 10.0, "sigma_min / sigma_max ~ 1e-5: judges the refinement"),
    Case("lowk", (41, 41), 2.0, "the same, lower still"),
    Case("lowk", (129, 129), 32.0, "ill conditioned and two tiles per workgroup"),
    Case("gv2", (5, 5), 5.0, "smallest 2D grid, Greengard-Vico"),
    Case("gv2", (7, 7), 7.0, "N = 49, Greengard-Vico"),
    Case("gv2", (129, 129), 10.0, "N = 16641 with the Greengard-Vico kernel"),
    Case("gv3", (4, 4, 4), None, "smallest 3D grid: LO, IN, HI stencils overlap, N = 64 is one full tile"),
    Case("gv3", (4, 6, 8), None, "smallest, three different axes"),
    Case("gv3", (8, 6, 4), None, "the same reversed"),
    Case("gv3", (10, 12, 18), None, "reversal of the (18, 12, 10) of test_gpu_sparsify.py"),
    Case("gv3", (16, 16, 16), 2.0, "low k in 3D"),
    Case("gv3", (26, 26, 26), None, "N = 17576: 275 chunks, tail of 40"),
    Case("gv3", (16, 32, 34), None, "N = 17408: 272 chunks, no tail, three different axes"),
    Case("gv3", (32, 32, 34), None, "N = 34816: 544 chunks, two to three tiles per workgroup"),
]
LOWK = [c for c in CASES if c.kind == "lowk"]


def case_id(case):
    k = "" if case.k is None else f"-k{case.k:g}"
    return f"{case.kind}-{'x'.join(str(v) for v in case.dims)}{k}"


def find(kind, dims, k=None):
    got = [c for c in CASES if (c.kind, c.dims, c.k) == (kind, tuple(dims), k)]
    assert len(got) == 1, (kind, dims, k)
    return got[0]


def tiles(case):
    """(chunks, tiles of the busiest workgroup, live columns of the last tile)"""
    N = int(np.prod(case.dims))
    chunks = -(-N // GCOLS)
    return chunks, -(-chunks // GPARTS), N - (chunks - 1) * GCOLS


# ---- nu without a symmetry: the Gaussian of the example drivers off centre, another width per axis, the same cut-off ------
def nu2(X, Y):
    return 0.3 * np.exp(-(55 * (X - 0.13) ** 2 + 30 * (Y + 0.21) ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48)


def nu3(X, Y, Z):
    return (0.3 * np.exp(-(55 * (X - 0.13) ** 2 + 30 * (Y + 0.21) ** 2 + 42 * (Z - 0.07) ** 2))
            * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48))


def nu2_other(X, Y):                                       # the field the set_nu test moves to
    return 0.2 * np.exp(-(25 * (X + 0.19) ** 2 + 60 * (Y - 0.11) ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48)


def nu3_other(X, Y, Z):
    return (0.2 * np.exp(-(25 * (X + 0.19) ** 2 + 60 * (Y - 0.11) ** 2 + 35 * (Z + 0.23) ** 2))
            * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48))


Geometry = collections.namedtuple("Geometry", "axes h k coords D0")


def geometry(case):
    """axes (x, y[, z]), h, k, the grid coordinates (X, Y[, Z], first axis fastest) and D0 (trapezoidal kinds)"""
    d = case.dims
    if case.kind in ("trap", "lowk"):                      # examples/example.jl: x = -a/2:h:a/2, one h for both axes
        h = 1.0 / (max(d) - 1)
        axes = tuple(h * (np.arange(v) - (v - 1) / 2.0) for v in d)
        k = 1.0 / h if case.k is None else case.k
        D = o.reference_vals_trap_rule()[1]
        D0 = D[0] if case.kind == "lowk" else D[int(round(k * h)) - 1]
        return Geometry(axes, h, k, o.grid2d(*axes), D0)
    h = 1.0 / d[0]                                         # examples/example3D.jl: x = -a/2:h:a/2-h
    axes = tuple(-0.5 + h * np.arange(v) for v in d)
    k = 1.0 / h if case.k is None else case.k
    return Geometry(axes, h, k, o.grid2d(*axes) if len(d) == 2 else o.grid3d(*axes), None)


def nu_of(case, other=False):
    g = geometry(case)
    f = (nu2_other if other else nu2) if len(case.dims) == 2 else (nu3_other if other else nu3)
    return np.asarray(f(*g.coords), dtype=np.float64)


def restatement_rows(case):
    g = geometry(case)
    if case.kind in ("trap", "lowk"):
        return ref.direct_rows(g.k, g.coords[0], g.coords[1], g.D0, g.h)
    if case.kind == "gv2":
        return ref.conv_rows(o.build_fast_convolution(g.axes[0], g.axes[1], g.h, g.k, nu2, quadRule="Greengard_Vico"))
    box = abs(g.axes[0][-1] - g.axes[0][0]) + g.h
    return ref.gv3d_rows(*case.dims, box, g.k)


def device_operator(pkg, case):
    """the plan under test, as a user makes it"""
    g = geometry(case)
    if case.kind == "trap":
        return pkg.buildFastConvolution(g.axes[0], g.axes[1], g.h, g.k, nu2, quadRule="trapezoidal")
    if case.kind == "lowk":
        from fast_solver_lippmann_schwinger_amd.sparsify import _direct_plan
        return _direct_plan(g.k, g.coords[0], g.coords[1], g.D0, *case.dims)
    if case.kind == "gv2":
        return pkg.buildFastConvolution(g.axes[0], g.axes[1], g.h, g.k, nu2, quadRule="Greengard_Vico")
    return pkg.buildFastConvolution3D(*g.axes, *g.coords, g.h, g.k, nu3)


def dims3(case):
    return tuple(case.dims) + (1,) * (3 - len(case.dims))


def build_with_figures(rows, dims3_, nu=None, k=None):
    """sparsify_ref.build plus refine[c] and row0[c] (module docstring)"""
    refine, row0 = [], []

    def per_class(c, R, Gs, U, s):
        corrected, uncorrected = ref.gram_refine(Gs)
        b = EPS * s[0] / (s[-2] - s[-1])
        refine.append((ref.phase_distance(corrected, U[:, -1]), ref.phase_distance(uncorrected, U[:, -1]), b))
        row0.append(R[0].copy())

    r = ref.build(rows, *dims3_, nu=nu, k=k, per_class=per_class)
    r["refine"], r["row0"] = np.array(refine), row0
    return r


@functools.lru_cache(maxsize=None)
def reference(case):
    """the restatement of one entry of CASES, computed once per process; read only"""
    g = geometry(case)
    with_nu = case.kind != "lowk"
    return build_with_figures(restatement_rows(case), dims3(case), nu=nu_of(case) if with_nu else None, k=g.k if with_nu else None)


def conditions(r):
    """(smallest sigma_-2 / sigma_min, smallest sigma_min / sigma_max) over the classes"""
    s = r["sigma"]
    return float((s[:, 1] / s[:, 2]).min()), float((s[:, 2] / s[:, 0]).min())


# ---- literal symbols (lsfc_plan_create_2d / 3d take any) ------------------------------------------------------------
# A random symbol on the (2n)^d grid times a Gaussian envelope: white noise alone gives classes whose smallest singular values
# are all alike (sigma_-2 / sigma_min < 1.2), under the envelope they spread.  Seed and width: the first pair tried whose
# axis-by-axis symmetrisation meets the input conditions in every class (test_sparsify_cases_cpu.py asserts them).
# The envelope alone makes the kernel smooth, and a_c G[S_c, S_c] then cancels: cancel_c = |G[S,S]|_2 / |a_c G[S,S]| (sparsify_ref.build)
# is 102 in 3D and 7.4 in 2D, so two vectors that both sit within b_c of the true one, as the SVD's and the device's do, give AG
# rows up to 102 b_c apart, and the numpy emulation itself is 6.5 ... 15.5 b_c off there: the reference cannot judge an AG row
# at tol_c, which is a bound on the vector.  The kernels of the builders have a strong self term; the literal symbols get one
# too, a constant SELF x the largest kernel entry added to the symbol (a unit source in the kernel: it enters G[S,S] only, the
# rows outside S_c and with them sigma and the vector are the same).  Input condition of these cases: cancel_c <= 2 in every
# class.  SELF: the smallest of 0, 1, 2, 4, 8 that meets it in both cases, measured on the CPU (3D: 102, 4.0, 1.67, 1.26, 1.13).
SELF = 2.0
MAX_CANCEL = 2.0
LITERAL = {(6, 8, 10): dict(seed=1, width=0.35, self=SELF), (9, 11): dict(seed=1, width=0.35, self=SELF)}


def literal_symbol(dims, symmetry):
    """reduced symbol in plain FFT order on the grid 2 * dims.  symmetry: "none"; "point": G(-k) = G(k) over all axes jointly,
    which makes the Green's matrix symmetric but not the kernel even per axis; "axes": symmetrised axis by axis (even)."""
    spec = LITERAL[tuple(dims)]
    grid = tuple(2 * v for v in dims)
    rng = np.random.default_rng(spec["seed"])
    G = rng.standard_normal(grid) + 1j * rng.standard_normal(grid)
    f = [np.fft.fftfreq(L) for L in grid]                  # cycles per sample, |f| <= 1/2
    q = sum((np.reshape(v, [-1 if a == b else 1 for b in range(len(grid))]) / spec["width"]) ** 2 for a, v in enumerate(f))
    G = G * np.exp(-q)
    G = G + spec["self"] * np.abs(np.fft.ifftn(G)).max()      # a constant in the symbol is a unit source in the kernel
    axes = tuple(range(len(grid)))
    if symmetry == "point":
        G = 0.5 * (G + np.roll(np.flip(G, axis=axes), 1, axis=axes))
    elif symmetry == "axes":
        for ax in axes:                                    # symmetrise of tests/test_gpu_apply_forms.py
            G = 0.5 * (G + np.roll(np.flip(G, axis=ax), 1, axis=ax))
    else:
        assert symmetry == "none"
    return G


def literal_nu(dims):
    return np.random.default_rng(5).uniform(-0.3, 0.3, int(np.prod(dims)))


LITERAL_OMEGA = 2.0


def literal_operator(pkg, dims, symmetry):
    G = np.fft.fftshift(literal_symbol(dims, symmetry))    # the constructors take the centred order
    g, nu = G.shape, literal_nu(dims)
    if len(dims) == 3:
        return pkg.FastM3D(G, nu, g[0], g[1], g[2], dims[0], dims[1], dims[2], LITERAL_OMEGA)
    return pkg.FastM(G, nu, g[0], g[1], dims[0], dims[1], LITERAL_OMEGA, quadRule="Greengard_Vico")


@functools.lru_cache(maxsize=None)
def literal_reference(dims):
    rows = ref.literal_rows(literal_symbol(dims, "axes"), dims)
    return build_with_figures(rows, tuple(dims) + (1,) * (3 - len(dims)), nu=literal_nu(dims), k=LITERAL_OMEGA)
