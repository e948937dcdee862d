"""Every form of the pruned axis passes (xfwd, yfwd, fused z, yinv, xinv of csrc/fft_kernels.hip) against the CPU oracle.

One plan per (shape, symmetry, padding); many ``set_tuning`` combinations on it, all compared with ONE oracle result per input
(``o.apply_reduced`` / ``o.convolve_reduced`` on seeded random nu, b and symbol).  After every ``set_tuning`` the test reads
``M.describe_passes()`` (lsfc_plan_describe_passes) and asserts that the form it asked for is the form that runs -- or, where
the dispatcher refuses a request, the substitute that include/lsfc.h documents.  No request passes unobserved.

Two assertions per case:
  1. the project's bound, rel-l2 error < TOL = 1e-10;
  2. a rounding-level bound: the error of every form is at most MARGIN = 8 times the error ``e_ref`` of the FORCE_ROCFFT plan
     of the same operator against the same oracle result.  That plan is rocFFT plus the pointwise kernels and shares no code
     with the passes tested here; both are double-precision transforms of the same depth and differ in factorisation order and
     twiddle generation, which moves the error by small factors.  A twiddle wrong in the twelfth digit or a symbol value taken
     from the neighbouring slot is orders of magnitude above it.  (Measured on the MI355X: the largest ratio of any form is 1.31, at 1536 points; the table per
     line length is in DESIGN.md next to the tolerance paragraph.  No family needs a margin of its own.)
The bare convolution (no nu, alpha = 0: another branch of the x passes only) is compared wherever the x passes change form and
once per plan elsewhere.

Out of scope: LSFC_Z_QUARTER and LSFC_NO_SIBLING_PAIRS are read once per process and cannot be toggled inside a test; the
distributed and host-pipeline drivers have their own files (test_gpu_distributed.py, test_gpu_apply.py::test_host_vector_pipeline).
"""
import itertools

import numpy as np
import pytest

from oracle import lsfc_oracle as o
from cases import TOL
from conftest import rel_err

pytestmark = pytest.mark.gpu
FORCE_ROCFFT = 2
MARGIN = 8.0
LENGTHS = [32, 48, 64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024, 1280, 1536, 2048]
SYMS = {"none": (), "z": (2,), "y": (1,), "yz": (1, 2), "xyz": (0, 1, 2), "xy": (0, 1)}     # ("xy": the even symbol of the 2D cases)
FUSED_SYMS = ["none", "z", "y", "yz", "xyz"]
ENV = ("LSFC_PAD1", "LSFC_PAD2", "LSFC_SYM_EVEN_Y", "LSFC_SYM_EVEN_Z", "LSFC_2D_TILED", "LSFC_SPLIT_X", "LSFC_SPLIT_S", "LSFC_SPLIT_Z",
       "LSFC_Z_HALF", "LSFC_TW_LDS", "LSFC_SYM_PREFETCH", "LSFC_YTILE_G", "LSFC_YTILE_Z", "LSFC_BATCH_FUSE", "LSFC_Z_PERSIST", "LSFC_XLANE")
DEFAULTS = dict(split_x=1, split_s=1, split_z=-1, sym_prefetch=-1, tw_lds=1, z_half=-1, z_persist=-1, xlane=-1, ytile_g=0, ytile_z=0, batch_fuse=-1)

# facts of the line lengths that the documented fallbacks depend on (include/lsfc.h):
# whole-complex exchanges of 8 lines, (L + L/8) * 8 * 16 bytes, exceed the 160 KiB of LDS from 1280 points on: forced split
FORCED_SPLIT = {1280, 1536, 2048}
# the lines whose persistent whole tiles (8 lines, whole-complex exchanges) have two consecutive stages of equal radix and so a
# lane exchange (knob "xlane"; include/lsfc.h): a fixed fact of each factorisation.  Everywhere else XL = 0 whatever is asked.
XLANE_WHOLE = {128, 192, 256, 320, 384, 512, 640, 768, 1024}
XLANE_HALF = {1024, 1280, 1536, 2048}              # the same for the ticketed half tiles (>= 1024 points)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def parse(text):
    """describe_passes() -> {"pipeline": str, "passes": [dict, ...] in launch order, "store": dict}"""
    lines = text.strip().split("\n")
    out = {"pipeline": lines[0].split("=", 1)[1], "passes": [], "store": {}}
    for ln in lines[1:]:
        tok = ln.split()
        if "=" in tok[0]:
            out["store"] = {k: (v if k == "batch" else int(v)) for k, v in (t.split("=") for t in tok)}
        else:
            d = {k: int(v) for k, v in (t.split("=") for t in tok[1:])}
            d["family"] = tok[0]
            out["passes"].append(d)
    return out


def pass_of(desc, prefix):
    got = [p for p in desc["passes"] if p["family"].startswith(prefix)]
    assert len(got) == 1, (prefix, desc)
    return got[0]


def expect(p, **want):
    got = {k: p[k] for k in want}
    assert got == want, (p, want)


def symmetrise(G, axes):
    for ax in axes:
        G = 0.5 * (G + np.roll(np.flip(G, axis=ax), 1, axis=ax))
    return G


class Case:
    """A random operator on the padded grid `grid` for the grid `dims`, its oracle results (computed once), the plan of the
    hand-written pipeline and the error of the rocFFT plan of the same operator against the same oracle results."""

    def __init__(self, lsfc, grid, dims, sym, seed, omega=2.0, nbatch=0, convolve=True):
        # nbatch: right-hand sides of the batch checks (0: none); convolve: also the bare convolution (the 2D FFTconvolution of
        # the reference exists for square grids only, so the 2D cases leave it out)
        rng = np.random.default_rng(seed)
        G2 = symmetrise(rng.standard_normal(grid) + 1j * rng.standard_normal(grid), SYMS[sym])
        N = int(np.prod(dims))
        self.dims, self.grid, self.omega = dims, grid, omega
        self.nu = rng.uniform(-0.3, 0.3, N)
        self.b = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        self.want = o.apply_reduced(G2, self.nu, omega, self.b, dims)
        self.wantc = o.convolve_reduced(G2, self.b, dims) if convolve else None
        self.B = np.stack([self.b] + [rng.standard_normal(N) + 1j * rng.standard_normal(N) for _ in range(nbatch - 1)]) if nbatch else None
        self.wantB = [self.want] + [o.apply_reduced(G2, self.nu, omega, v, dims) for v in self.B[1:]] if nbatch else None
        self.lsfc = lsfc
        self._G = np.fft.fftshift(G2)
        self.M = self.plan(0)
        Mr = self.plan(FORCE_ROCFFT)
        assert self.M.pipeline == "pruned-hip" and Mr.pipeline == "rocfft-reduced"
        assert self.M.padded_dims[:len(grid)] == tuple(grid)
        assert parse(Mr.describe_passes()) == {"pipeline": "rocfft-reduced", "passes": [], "store": {}}
        self.e_ref = rel_err(Mr * self.b, self.want)
        self.e_refc = rel_err(lsfc.FFTconvolution(Mr, self.b), self.wantc) if convolve else None
        Mr.close()

    def plan(self, flags):
        g, d = self.grid, self.dims
        if len(d) == 3:
            return self.lsfc.FastM3D(self._G, self.nu, g[0], g[1], g[2], d[0], d[1], d[2], self.omega, flags=flags)
        return self.lsfc.FastM(self._G, self.nu, g[0], g[1], d[0], d[1], self.omega, quadRule="Greengard_Vico", flags=flags)

    def tune(self, **knobs):
        """set_tuning on top of the defaults; returns the parsed description"""
        self.M.set_tuning(**{**DEFAULTS, **knobs})
        return parse(self.M.describe_passes())

    def _judge(self, got, want, e_ref, what):
        err = rel_err(got, want)
        assert err < TOL, (what, err)
        assert err <= MARGIN * e_ref, (what, err, e_ref, err / e_ref)

    def check(self, what, convolve=False):
        y = self.M * self.b
        self._judge(y, self.want, self.e_ref, what)
        if convolve:
            self._judge(self.lsfc.FFTconvolution(self.M, self.b), self.wantc, self.e_refc, what + " conv")
        return y

    def check_batch(self, what):
        Y = self.lsfc.apply_batch(self.M, self.B, 0)
        for r, w in enumerate(self.wantB):
            self._judge(Y[r], w, self.e_ref, f"{what} rhs{r}")


# ---------------------------------------------------------------------------- a. the fused pass, 3D
def z_case(lsfc, L, short, sym, nbatch=3):
    # n = m = 16: 4 tiles x 32 rows = 128 tiles in row pairs, so the ticketed forms are legal
    c = Case(lsfc, (32, 32, L), (16, 16, L // 2 - short), sym, seed=1000 * L + 10 * short + len(sym), nbatch=nbatch)
    d = parse(c.M.describe_passes())
    axes = SYMS[sym]
    expect(d["store"], ytab=int(1 in axes), zmirror=int(2 in axes), sym_rows=17 if 1 in axes else 32, sym_hz=L // 2 + 8 if 2 in axes else L,
           pitch1=32, pitch2=8 * (L // 2 - short))
    return c


def one_tile_expect(L, ze, full, sp, pf, tw, batch):
    """the one-tile-per-workgroup kernel asked for by split_z / sym_prefetch / tw_lds with z_persist = 0, z_half = 0"""
    if L == 2048:
        # whole 8-line tiles of the 2048-point line do not fit the LDS: whole-complex half tiles whatever the knobs say,
        # a batch member by member
        return dict(family="zfused_half", SPLIT=0, PREFETCH=0, TWL=0, LINES=4, WPE=2, ZE=ze, FULL=full, BATCH=0, PER_MEMBER=int(batch))
    split = 1 if L in FORCED_SPLIT else sp
    return dict(family="zfused", SPLIT=split, PREFETCH=0 if batch else pf, TWL=tw, LINES=8, WPE=1, ZE=ze, FULL=full, BATCH=int(batch), PER_MEMBER=0)


@pytest.mark.parametrize("sym", FUSED_SYMS)
@pytest.mark.parametrize("short", [0, 6])
@pytest.mark.parametrize("L", LENGTHS)
def test_fused_pass_one_tile_forms(lsfc, L, short, sym):
    c = z_case(lsfc, L, short, sym)
    ze, full = int(2 in SYMS[sym]), int(short == 0)
    first = True
    for sp, pf, tw in itertools.product((0, 1), (0, 1), (0, 1)):
        knobs = dict(z_persist=0, z_half=0, split_z=sp, sym_prefetch=pf, tw_lds=tw, batch_fuse=1)
        d = c.tune(**knobs)
        expect(pass_of(d, "zfused"), **one_tile_expect(L, ze, full, sp, pf, tw, False))
        expect(d["store"], batch="none")
        c.check(f"one-tile sp={sp} pf={pf} tw={tw}", convolve=first)
        first = False
        # three right-hand sides in one launch per pass (BATCH kernels); at 2048 points the fused pass member by member
        d3 = parse(c.M.describe_passes(3))
        expect(pass_of(d3, "zfused"), **one_tile_expect(L, ze, full, sp, pf, tw, True))
        expect(d3["store"], batch="fused")
        c.check_batch(f"one-tile sp={sp} pf={pf} tw={tw} batch")
    # batch_fuse = 0: the whole pipeline member by member
    c.tune(z_persist=0, batch_fuse=0)
    expect(parse(c.M.describe_passes(3))["store"], batch="per_member")
    c.check_batch("batch_fuse=0")


HALF_FLAVOUR = {1: (0, 1), 2: (1, 1), 3: (1, 0), 4: (0, 0)}       # z_half -> (SPLIT, PREFETCH)


@pytest.mark.parametrize("sym", ["none", "xyz"])
@pytest.mark.parametrize("short", [0, 6])
@pytest.mark.parametrize("L", [1024, 1536])
def test_fused_pass_half_tile_flavours(lsfc, L, short, sym):
    c = z_case(lsfc, L, short, sym)
    ze, full = int(sym == "xyz"), int(short == 0)
    for zh in range(5):
        d = c.tune(z_persist=0, z_half=zh, batch_fuse=1)
        z = pass_of(d, "zfused")
        if zh == 0:
            expect(z, family="zfused", LINES=8)
        else:
            sp, pf = HALF_FLAVOUR[zh]
            expect(z, family="zfused_half", LINES=4, SPLIT=sp, PREFETCH=pf, ZE=ze, FULL=full, TWL=0, WPE=(3 if zh == 3 else 2) if L == 1024 else 1)
            # the half-tile forms take one right-hand side per launch
            expect(pass_of(parse(c.M.describe_passes(3)), "zfused"), family="zfused_half", PER_MEMBER=1, BATCH=0, SPLIT=sp, PREFETCH=pf)
        c.check(f"z_half={zh}")
        c.check_batch(f"z_half={zh} batch")
    # auto: 1024 points -- 2 for a full symbol, whole tiles for a z-even one; 1536 points -- 1
    z = pass_of(c.tune(z_persist=0), "zfused")
    if L == 1024:
        expect(z, **(dict(family="zfused", LINES=8) if ze else dict(family="zfused_half", SPLIT=1, PREFETCH=1)))
    else:
        expect(z, family="zfused_half", SPLIT=0, PREFETCH=1)
    c.check("z_half=auto")


def persist_xl(L, req, twl, tickets):
    """lane-exchange form of the persistent whole-tile kernels (include/lsfc.h: 3 and 5 need the twiddle table, 5 the tickets)"""
    if L not in XLANE_WHOLE:
        return 0
    if req <= 1:
        return req
    if not twl:
        return 0
    return 5 if (req == 5 and tickets) else (3 if req == 3 else 1)


def persist_expect(L, zp, xl, tw, z_half_off=False):
    """what z_persist = zp runs as on a z-even symbol with 128 tiles in row pairs (one right-hand side)"""
    half = dict(family="zfused_persist_half", LINES=4, SPLIT=0, TWL=1, LATE_SYM=1, TICKETS=1, XL=int(xl != 0 and L in XLANE_HALF))
    if zp == 5 and L >= 1024:
        return half
    if L == 2048 or (L == 1536 and not z_half_off):
        # only half tiles of these lines run (LDS at 2048 points, registers at 1536): every other persistent form gives way to
        # the one-tile half-tile kernel
        return dict(family="zfused_half", LINES=4, TICKETS=0, LATE_SYM=0, SPLIT=0)
    forced = L in FORCED_SPLIT
    if zp in (1, 2):
        e = dict(SPLIT=int(zp == 2 or forced), LATE_SYM=0, TICKETS=0)
    elif zp == 4 or zp == 5 or forced:          # 5 below 1024 points runs as 4
        e = dict(SPLIT=1, LATE_SYM=1, TICKETS=0)
    else:
        e = dict(SPLIT=0, LATE_SYM=1, TICKETS=int(zp == 6))
    e["TWL"] = tw
    e["XL"] = persist_xl(L, xl, e["TWL"], e["TICKETS"]) if (e["LATE_SYM"] and not e["SPLIT"]) else 0
    return dict(family="zfused_persist", LINES=8, **e)


@pytest.mark.parametrize("sym", ["z", "xyz"])
@pytest.mark.parametrize("short", [0, 6])
@pytest.mark.parametrize("L", LENGTHS)
def test_fused_pass_persistent_forms(lsfc, L, short, sym):
    c = z_case(lsfc, L, short, sym, nbatch=0)
    full = int(short == 0)
    seen = set()
    for zp, xl, tw in itertools.product(range(1, 7), (0, 1, 3, 5), (0, 1)):
        z = pass_of(c.tune(z_persist=zp, xlane=xl, tw_lds=tw), "zfused")
        expect(z, ZE=1, FULL=full, PER_MEMBER=0, BATCH=0, **persist_expect(L, zp, xl, tw))
        y = c.check(f"z_persist={zp} xlane={xl} tw_lds={tw}")
        seen.add(z["family"])
        if z["TICKETS"]:
            # tickets are fresh per launch: a second apply draws the same tiles and gives the same bits
            assert np.array_equal(c.M * c.b, y), (zp, xl, tw)
    if L >= 1024:
        assert "zfused_persist_half" in seen
    if L == 1536:
        # with the half-tile one-tile form switched off the persistent whole tiles run, split (221 KiB whole complex)
        for zp in (1, 2, 3, 4, 6):
            z = pass_of(c.tune(z_persist=zp, z_half=0), "zfused")
            expect(z, **persist_expect(L, zp, 1, 1, z_half_off=True))
            c.check(f"z_persist={zp} z_half=0")


# ---------------------------------------------------------------------------- b. the x and y passes
@pytest.mark.parametrize("s", [0, 3])
@pytest.mark.parametrize("L", LENGTHS)
def test_x_pass_forms(lsfc, L, s):
    c = Case(lsfc, (L, 32, 32), (L // 2 - s, 16, 16), "none", seed=7 * L + s)
    for sx in (0, 1):
        d = c.tune(split_x=sx)
        for fam in ("xfwd", "xinv"):
            expect(pass_of(d, fam), SPLIT=sx, FULL=int(s == 0), L=L)
        c.check(f"split_x={sx}", convolve=True)


def tile_expect(want, auto, size):
    """the y passes' block-order tile: the request (0: auto), clipped to the grid, rounded down to a divisor"""
    t = min(want if want > 0 else auto, size)
    while size % t:
        t -= 1
    return t


@pytest.mark.parametrize("s", [0, 3])
@pytest.mark.parametrize("L", LENGTHS)
def test_y_pass_forms(lsfc, L, s):
    c = Case(lsfc, (64, L, 32), (32, L // 2 - s, 12), "none", seed=11 * L + s)
    forced = None
    for ss in (0, 1):
        d = c.tune(split_s=ss)
        for fam in ("yfwd", "yinv"):
            p = pass_of(d, fam)
            expect(p, FULL=int(s == 0), L=L, SPLIT=int(ss or p["FORCED_SPLIT"]))
            forced = p["FORCED_SPLIT"]
            # whole-complex exchanges of the workgroup's lines, (L + L/8) * LINES * 16 bytes, must fit the 160 KiB of LDS
            assert forced == int((L + L // 8) * p["LINES"] * 16 > 160 * 1024), p
        c.check(f"split_s={ss}", convolve=True)
    assert forced == int(L in FORCED_SPLIT)
    ngrp = 64 // pass_of(d, "yfwd")["LINES"]
    for tg, tz in itertools.product((0, 1, 2, 3, 8), (0, 1, 5, 8)):
        d = c.tune(ytile_g=tg, ytile_z=tz)
        for fam in ("yfwd", "yinv"):
            # auto: all groups x 1 plane, from 1024 points on 32 groups x 8 planes (clipped: 8 groups, 6 planes of 12)
            expect(pass_of(d, fam), TG=tile_expect(tg, 32 if L >= 1024 else ngrp, ngrp), TZ=tile_expect(tz, 8 if L >= 1024 else 1, 12))
        c.check(f"ytile={tg}x{tz}")


@pytest.mark.parametrize("pads", [(0, 0), (40, 72), (8, 8)])
@pytest.mark.parametrize("shape", [((64, 96, 32), (32, 45, 12)), ((48, 32, 64), (24, 16, 29))])
def test_row_paddings(lsfc, shape, pads, monkeypatch):
    # LSFC_PAD1 / LSFC_PAD2 are read at plan creation: the pitch of the A1 rows and of the A2 tile rows
    monkeypatch.setenv("LSFC_PAD1", str(pads[0]))
    monkeypatch.setenv("LSFC_PAD2", str(pads[1]))
    grid, dims = shape
    c = Case(lsfc, grid, dims, "xyz", seed=sum(grid) + pads[0])
    d = parse(c.M.describe_passes())
    expect(d["store"], pitch1=grid[0] + pads[0], pitch2=8 * dims[2] + pads[1], ytab=1, zmirror=1)
    for sx, ss, zp in itertools.product((0, 1), (0, 1), (0, 3)):
        d = c.tune(split_x=sx, split_s=ss, z_persist=zp)
        expect(pass_of(d, "xfwd"), SPLIT=sx)
        expect(pass_of(d, "yinv"), SPLIT=ss)
        expect(pass_of(d, "zfused"), family="zfused_persist" if zp else "zfused")
        c.check(f"pads={pads} split_x={sx} split_s={ss} z_persist={zp}", convolve=True)


@pytest.mark.parametrize("tiled", ["0", "1"])
@pytest.mark.parametrize("dims", [(40, 93), (64, 128)])
def test_2d_geometries(lsfc, dims, tiled, monkeypatch):
    # 2D: xfwd -> fused pass along y -> xinv on natural rows or on tiles (LSFC_2D_TILED), a mixed-radix (80 x 192) and a
    # power-of-two (128 x 256) grid, even symbol
    monkeypatch.setenv("LSFC_2D_TILED", tiled)
    grid = tuple({40: 80, 93: 192, 64: 128, 128: 256}[v] for v in dims)
    c = Case(lsfc, grid, dims, "xy", seed=sum(dims), convolve=False)
    d = parse(c.M.describe_passes())
    # tiles need whole groups of 8 tiles: 80 / 8 = 10 tiles keep the natural rows
    want_tiles = tiled == "1" and (grid[0] // 8) % 8 == 0
    assert (d["store"]["tile2d"] > 0) == want_tiles and d["store"]["zmirror"] == 1
    assert [p["family"] for p in d["passes"]] == ["xfwd", "zfused", "xinv"]
    for sx, sp in itertools.product((0, 1), (0, 1)):
        d = c.tune(split_x=sx, split_z=sp)
        expect(pass_of(d, "xfwd"), SPLIT=sx, FULL=int(2 * dims[0] == grid[0]))
        expect(pass_of(d, "xinv"), SPLIT=sx)
        expect(pass_of(d, "zfused"), family="zfused", SPLIT=sp, ZE=1, FULL=int(2 * dims[1] == grid[1]))
        c.check(f"2d tiled={tiled} split_x={sx} split_z={sp}")


# ---------------------------------------------------------------------------- c. the size-chosen defaults, nothing forced
def test_default_row_padding_and_block_order_from_1024_point_y_lines(lsfc):
    # pads[1] = 1024: rows padded by 40 / 72 elements, y-pass block order 32 x 8 clipped to the grid (8 groups, 16 planes)
    c = Case(lsfc, (64, 1024, 32), (32, 512, 16), "xyz", seed=5)
    d = parse(c.M.describe_passes())
    expect(d["store"], pitch1=64 + 40, pitch2=8 * 16 + 72, ytab=1, zmirror=1)
    for fam in ("yfwd", "yinv"):
        expect(pass_of(d, fam), TG=8, TZ=8, SPLIT=1, FULL=1)
    c.check("defaults", convolve=True)


@pytest.mark.parametrize("m,family", [(64, "zfused_persist"), (48, "zfused")])
def test_persistent_form_from_4096_tiles_on(lsfc, m, family):
    # 256 / 8 = 32 tiles per row x 128 or 96 rows: 4096 and 3072 tiles, either side of the threshold
    c = Case(lsfc, (256, 2 * m, 32), (128, m, 16), "xyz", seed=m)
    z = pass_of(parse(c.M.describe_passes()), "zfused")
    expect(z, family=family, ZE=1, FULL=1)
    if family == "zfused_persist":
        expect(z, SPLIT=0, LATE_SYM=1, TICKETS=0, LINES=8)        # auto below 1024 points: form 3
    c.check("defaults")


@pytest.mark.parametrize("L,form", [(1024, 6), (1280, 5), (1536, 5), (2048, 5)])
def test_full_size_default_forms_on_small_grids(lsfc, L, form):
    # (16, 16, L/2): the lines of 512^3, 640^3, 768^3 and 1024^3 on 128 tiles.  With nothing forced there are too few tiles for
    # the persistent form; then the form those sizes choose by default (z_persist = -1 resolves to `form`), forced
    c = Case(lsfc, (32, 32, L), (16, 16, L // 2), "xyz", seed=L)
    z = pass_of(parse(c.M.describe_passes()), "zfused")
    assert not z["family"].startswith("zfused_persist"), z
    expect(z, family="zfused_half" if L in (1536, 2048) else "zfused", ZE=1, FULL=1)
    c.check("defaults")
    z = pass_of(c.tune(z_persist=form), "zfused")
    if form == 6:
        # 512^3: ticketed whole tiles, lane exchanges with row pairs as work items (xlane auto = 5)
        expect(z, family="zfused_persist", TICKETS=1, LATE_SYM=1, SPLIT=0, TWL=1, XL=5, LINES=8)
    else:
        expect(z, family="zfused_persist_half", TICKETS=1, LATE_SYM=1, SPLIT=0, TWL=1, LINES=4, XL=1)
    y = c.check(f"z_persist={form}")
    assert np.array_equal(c.M * c.b, y)


# ---------------------------------------------------------------------------- d. storage switches
@pytest.mark.parametrize("even_y,even_z", [("0", None), (None, "0"), ("0", "0")])
def test_symbol_storage_switches(lsfc, even_y, even_z, monkeypatch):
    # LSFC_SYM_EVEN_Y=0 / LSFC_SYM_EVEN_Z=0: full storage although the symbol is even
    if even_y is not None:
        monkeypatch.setenv("LSFC_SYM_EVEN_Y", even_y)
    if even_z is not None:
        monkeypatch.setenv("LSFC_SYM_EVEN_Z", even_z)
    c = Case(lsfc, (32, 48, 80), (16, 21, 40), "xyz", seed=3)
    d = parse(c.M.describe_passes())
    expect(d["store"], ytab=int(even_y is None), zmirror=int(even_z is None), sym_rows=25 if even_y is None else 48,
           sym_hz=48 if even_z is None else 80)
    expect(pass_of(d, "zfused"), ZE=int(even_z is None))
    for zp in (0, 3):
        z = pass_of(c.tune(z_persist=zp), "zfused")
        # the persistent forms need the z-even half symbol
        expect(z, family="zfused_persist" if (zp and even_z is None) else "zfused")
        c.check(f"even_y={even_y} even_z={even_z} z_persist={zp}", convolve=True)


# ---------------------------------------------------------------------------- e. the knobs: environment route = set_tuning route
_OPERANDS = {}


def operands(grid, dims, axes):
    """a random symbol on `grid`, even along `axes`, with nu and b for `dims`; built once (no oracle: the two routes are compared with each other)"""
    key = (grid, dims, axes)
    if key not in _OPERANDS:
        rng = np.random.default_rng(sum(grid) + sum(dims))
        G = np.fft.fftshift(symmetrise(rng.standard_normal(grid) + 1j * rng.standard_normal(grid), axes))
        N = int(np.prod(dims))
        _OPERANDS[key] = (G, rng.uniform(-0.3, 0.3, N), rng.standard_normal(N) + 1j * rng.standard_normal(N))
    return _OPERANDS[key]


class Routes:
    """plans of one operator, their knobs set through the environment at creation or through set_tuning afterwards"""

    def __init__(self, lsfc, monkeypatch, shape):
        # "z": z_case at 1024 points, 6 short of a full line; "cube": 16^3
        self.grid, self.dims = {"z": ((32, 32, 1024), (16, 16, 506)), "cube": ((32, 32, 32), (16, 16, 16))}[shape]
        self.G, self.nu, self.b = operands(self.grid, self.dims, (0, 1, 2))
        self.lsfc, self.mp = lsfc, monkeypatch

    def plan(self, env=None, **knobs):
        for k, v in (env or {}).items():
            self.mp.setenv(k, v)
        M = self.lsfc.FastM3D(self.G, self.nu, *self.grid, *self.dims, 2.0)
        for k in env or {}:
            self.mp.delenv(k)
        M.set_tuning(**knobs)
        assert M.pipeline == "pruned-hip"
        return M

    def look(self, M):
        """what the plan runs for 1 and 3 right-hand sides, and M * b"""
        got = (M.describe_passes(1), M.describe_passes(3), M * self.b)
        M.close()
        return got


# knob -> (shape, value, knobs that both routes set beside it so that it bites)
KNOB_CASES = {
    "split_x": ("cube", 0, {}), "split_s": ("cube", 0, {}), "ytile_g": ("cube", 1, {}), "ytile_z": ("cube", 2, {}), "batch_fuse": ("cube", 0, {}),
    "split_z": ("z", 1, {}), "sym_prefetch": ("z", 0, {}), "tw_lds": ("z", 0, {}), "z_half": ("z", 1, {}), "z_persist": ("z", 3, {}),
    # the lane exchanges are a choice of the persistent forms only: the ticketed whole tiles (auto there: 5)
    "xlane": ("z", 0, {"z_persist": 6}),
}
assert set(KNOB_CASES) == set(DEFAULTS)


@pytest.mark.parametrize("knob", sorted(KNOB_CASES))
def test_knob_from_environment_equals_set_tuning(lsfc, monkeypatch, knob):
    shape, v, beside = KNOB_CASES[knob]
    R = Routes(lsfc, monkeypatch, shape)
    knobs = {**beside, knob: v}
    env1, env3, yenv = R.look(R.plan(env={"LSFC_" + k.upper(): str(val) for k, val in knobs.items()}))
    set1, set3, yset = R.look(R.plan(**knobs))
    base1, base3, _ = R.look(R.plan(**beside))
    assert env1 == set1 and env3 == set3, (knob, env1, set1, env3, set3)
    assert np.array_equal(yenv, yset), knob
    # the knob bites at this shape: wired to another field, neither route would change what runs
    assert (set1, set3) != (base1, base3), (knob, set1, set3)


def test_knob_parsing_edges(lsfc, monkeypatch):
    R = Routes(lsfc, monkeypatch, "cube")
    base1, base3, ybase = R.look(R.plan())
    assert pass_of(parse(base1), "xfwd")["SPLIT"] == 1 and pass_of(parse(base1), "zfused")["SPLIT"] == 1      # the defaults at 32 points
    # a flag: empty keeps the default, "y" is true, anything else is false
    assert R.look(R.plan(env={"LSFC_SPLIT_X": ""}))[:2] == (base1, base3)
    d1, d3, y = R.look(R.plan(env={"LSFC_SPLIT_X": "y"}))
    assert (d1, d3) == R.look(R.plan(split_x=1))[:2] and pass_of(parse(d1), "xfwd")["SPLIT"] == 1
    d1, d3, y = R.look(R.plan(env={"LSFC_SPLIT_X": "n"}))
    assert (d1, d3) == R.look(R.plan(split_x=0))[:2] and pass_of(parse(d1), "xfwd")["SPLIT"] == 0
    # an integer: atoi of whatever is set, so empty is 0 -- whole-complex exchanges where auto (-1) splits
    d1, d3, y = R.look(R.plan(env={"LSFC_SPLIT_Z": ""}))
    s1, s3, ys = R.look(R.plan(split_z=0))
    assert (d1, d3) == (s1, s3) and pass_of(parse(d1), "zfused")["SPLIT"] == 0 and np.array_equal(y, ys)
    # the row paddings are read at plan creation only; an unknown key
    M = R.plan()
    for key in ("pad1", "no_such_knob"):
        with pytest.raises(lsfc._lib.LsfcError, match="unknown tuning key") as e:
            M.set_tuning(**{key: 8})
        assert e.value.code == lsfc._lib.LSFC_EINVAL
    assert (M.describe_passes(1), M.describe_passes(3)) == (base1, base3)
    M.close()


# ---------------------------------------------------------------------------- f. the stages of the profile = the apply
STAGES = {"pruned-hip": ["xfwd", "yfwd", "zfused", "yinv", "xinv"], "rocfft-reduced": ["embed", "rocfft_fwd", "symbol_mul", "rocfft_inv", "crop_axpy"]}


@pytest.mark.parametrize("dims,pipeline,names", [((16, 12, 10), "pruned-hip", STAGES["pruned-hip"]), ((5, 4, 3), "rocfft-reduced", STAGES["rocfft-reduced"]),
                                                 ((24, 20), "pruned-hip", ["xfwd", "yfused", "xinv"])])
def test_profile_stages_are_the_apply(lsfc, dims, pipeline, names):
    import torch
    grid = tuple(2 * v for v in dims)
    G, nu, b = operands(grid, dims, tuple(range(len(dims))))          # even in every axis: M.T and M.H exist
    if len(dims) == 3:
        M = lsfc.FastM3D(G, nu, *grid, *dims, 2.0)
    else:
        M = lsfc.FastM(G, nu, *grid, *dims, 2.0, quadRule="Greengard_Vico")
    assert M.pipeline == pipeline
    x = torch.from_numpy(b).cuda()
    for V in (M, M.T, M.H):
        want = V * x
        y = torch.full_like(x, float("nan"))
        stages = lsfc.profile_apply(V, x, y, reps=1)
        assert [s[0] for s in stages] == names, stages
        assert all(nbytes > 0 and ms >= 0 for _, ms, nbytes in stages), stages
        assert torch.equal(y, want)
    # nu, 8 B per point, is counted in the pass that multiplies by it: the first stage of M, the last of M.T and M.H
    N = M.N
    sN, sT = lsfc.profile_apply(M, x, y, reps=1), lsfc.profile_apply(M.T, x, y, reps=1)
    assert sN[0][2] - sT[0][2] == 8 * N and sT[-1][2] - sN[-1][2] == 8 * N
    M.close()
