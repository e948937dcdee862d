"""GPU tests of a complex nu (lsfc_plan_set_nu_complex; an absorbing medium) against tests/complex_nu_ref.py.

Reference: a copy of the oracle operator with a complex nu for M, want_T(b) = b + omega^2 nu .* conv(b) and want_H(b) =
conj(want_T(conj b)) with the bare oracle convolution (tests/test_complex_nu_ref_cpu.py pins all three against the dense A, A.T and
A.conj().T).  Tolerances are the project's: rel-l2 error < TOL = 1e-10 (tests/cases.py), and at most MARGIN = 8 times e_ref,
the error of the FORCE_ROCFFT plan's FORWARD apply with Re nu against the oracle -- a path whose arithmetic a complex nu does
not touch (margin and reference of tests/test_gpu_apply_forms.py and tests/test_gpu_adjoint.py).  A bare convolution (the
trapezoidal FFTconvolution, mode 2 of apply_batch, a row of lsfc_sample_sources) has no identity term to be accurate against, so
it is read against e_refc, the error of the same FORCE_ROCFFT plan's convolution with Re nu, as tests/test_gpu_apply_forms.py
does with its `e_refc`.

The test nu has real part U(-0.3, 0.3) and imaginary part U(-0.2, 0.2), independent and of both signs, so that a swapped,
dropped or wrongly conjugated part shows at first order; the batch / host-vector case also has exact zeros and purely
imaginary entries."""
import ctypes as C

import numpy as np
import pytest

from oracle import lsfc_oracle as o
import bicgstabl_ref as br
import blocktri_cases as bc
import cases
import complex_nu_ref as cr
import krylov_common as kc
import sparsify_ref as sref
from cases import TOL
from conftest import rel_err
from test_gpu_adjoint import (ENV, FORCE_ROCFFT, LITERAL, PIPE, X_CASES, Sym, built, e_ref_of, get_op, judge, make, solver_setup, view)
from test_gpu_apply_forms import expect, parse, pass_of
import test_gpu_sparsify as gsp

pytestmark = pytest.mark.gpu
ALL = ("N", "T", "H")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def complex_part(rng, N):
    return rng.uniform(-0.2, 0.2, N)


class CSym(Sym):
    """Sym (a random operator with an even symbol, its plan with the real nu, e_ref of that real nu) plus a complex nu with
    the same real part and the references for it.  The plan takes the complex nu at `go_complex`."""

    def __init__(self, lsfc, grid, dims, seed, special=False):
        super().__init__(lsfc, grid, dims, seed)
        rng = np.random.default_rng(seed + 1000)
        self.nu_c = self.nu + 1j * complex_part(rng, self.N)
        if special:                                             # exact zeros and purely imaginary entries
            self.nu_c[::7] = 0.0
            self.nu_c[3::11] = 1j * self.nu_c[3::11].imag
        self.cref = cr.ref_of_reduced(self.G2, self.dims, self.nu_c, self.omega)
        self.cwant = {w: self.cref.of(w)(self.b) for w in ALL}
        self.e_ref                                              # (measured now, while the plan's nu is still real)
        self._e_refc = None

    @property
    def e_refc(self):
        """the yardstick of a bare convolution: G (Re nu .* b) on the FORCE_ROCFFT plan against the oracle"""
        if self._e_refc is None:
            Mr = self.plan(FORCE_ROCFFT)
            assert Mr.pipeline == "rocfft-reduced"
            self._e_refc = rel_err(self.lsfc.apply_batch(Mr, self.b[None, :], 2)[0], self.cref.conv(self.nu * self.b))
            Mr.close()
        return self._e_refc

    def go_complex(self):
        self.M.set_nu(self.nu_c)
        assert self.M.nu_is_complex and self.M.nu.dtype == np.complex128
        return self


# ---------------------------------------------------------------------------- 1. the builders, every pipeline
def make_complex(lsfc, name, flags, nu):
    Mo = built(name)["Mo"]
    if name == "gv16k10":
        n = built(name)["c"]["n"]
        return lsfc.FastM3D(Mo.GFFT, nu, Mo.ne, Mo.me, Mo.le, n, n, n, Mo.omega, flags=flags)
    return lsfc.FastM(Mo.GFFT, nu, Mo.ne, Mo.me, Mo.n, Mo.m, Mo.omega, quadRule=Mo.quadRule, flags=flags)


_CBUILT = {}


def cbuilt(name):
    if name not in _CBUILT:
        B = built(name)
        nu = cr.as_complex(B["Mo"].nu) * (1 - 0.5j)
        ref = cr.ref_of_oracle(B["Mo"], nu)
        _CBUILT[name] = dict(nu=nu, ref=ref, want={w: ref.of(w)(B["b"]) for w in ALL})
    return _CBUILT[name]


@pytest.mark.parametrize("flags", [0, LITERAL, FORCE_ROCFFT])
@pytest.mark.parametrize("name", ["trap21", "gv33", "gv32", "gv16k10"])
def test_builders_every_pipeline(lsfc, name, flags):
    B, Cx = built(name), cbuilt(name)
    M = make_complex(lsfc, name, flags, Cx["nu"])
    assert M.pipeline == PIPE[flags] and M.nu_is_complex and M.nu.dtype == np.complex128
    e_ref = e_ref_of(lsfc, name)
    for w in ALL:
        judge(view(M, w) * B["b"], Cx["want"][w], e_ref, f"{name} {M.pipeline} {w}")
    # the wrong conjugation is far away: the test can tell them apart
    assert rel_err(Cx["want"]["H"], np.conj(Cx["want"]["T"])) > 1e-3
    if name == "trap21":
        # the nu quirk of the trapezoidal FFTconvolution: G (nu .* b) with nu itself
        Mr = make(lsfc, name, FORCE_ROCFFT)
        e_refc = rel_err(lsfc.FFTconvolution(Mr, B["b"]), o.fft_convolution(B["Mo"], B["b"]))
        Mr.close()
        got = lsfc.FFTconvolution(M, B["b"])
        judge(got, o.fft_convolution(cr.with_nu(B["Mo"], Cx["nu"]), B["b"]), e_refc, f"{name} {M.pipeline} FFTconvolution")
    assert get_op(lsfc, M) == 0 and M.nu_is_complex
    M.close()


# ---------------------------------------------------------------------------- 2. the forms of the x passes
@pytest.mark.parametrize("case", sorted(X_CASES))
def test_x_pass_forms(lsfc, case, monkeypatch):
    import torch
    dims, grid, tiled = X_CASES[case]
    if tiled is not None:
        monkeypatch.setenv("LSFC_2D_TILED", tiled)
    c = CSym(lsfc, grid, dims, seed=sum(dims) + len(case))
    pruned = len(dims) == 2 or min(dims[1:]) >= 8
    assert c.M.pipeline == ("pruned-hip" if pruned else "rocfft-reduced")
    before = c.M.describe_passes()
    c.go_complex()
    assert c.M.describe_passes() == before                      # nu changes no form
    for sx in (0, 1):
        c.M.set_tuning(split_x=sx)
        d = parse(c.M.describe_passes())
        for fam in ("xfwd", "xinv") if pruned else ():
            expect(pass_of(d, fam), SPLIT=sx, FULL=int(2 * dims[0] == grid[0]), L=grid[0])
        for w in ALL:
            z = torch.from_numpy(c.b).cuda()
            out = view(c.M, w).mul_(z, z)                       # in place on the device: y aliases x
            assert out is z
            judge(z.cpu().numpy(), c.cwant[w], c.e_ref, f"{case} split_x={sx} {w}")
            assert np.array_equal((view(c.M, w) * torch.from_numpy(c.b).cuda()).cpu().numpy(), z.cpu().numpy()), (case, sx, w)
    assert c.M.describe_passes() == before
    c.M.close()


# ---------------------------------------------------------------------------- 3. batches
@pytest.fixture(scope="module", params=[(13, 7, 5), (13, 11, 9)], ids=["13x7x5-rocfft", "13x11x9-pruned"])
def small(lsfc, request):
    c = CSym(lsfc, (32, 32, 32), request.param, seed=77, special=True)
    c.pruned = request.param == (13, 11, 9)
    assert c.M.pipeline == ("pruned-hip" if c.pruned else "rocfft-reduced")
    assert np.count_nonzero(c.nu_c == 0) > 10 and np.count_nonzero((c.nu_c.real == 0) & (c.nu_c.imag != 0)) > 10
    c.y_real = {w: view(c.M, w) * c.b for w in ALL}             # the plan with its real nu, before it ever saw a complex one
    c.go_complex()
    rng = np.random.default_rng(78)
    c.B = np.stack([c.b] + [rng.standard_normal(c.N) + 1j * rng.standard_normal(c.N) for _ in range(10)])
    c.wantB = {w: [c.cref.of(w)(v) for v in c.B] for w in ALL}
    c.wantB["G nu"] = [c.cref.conv(c.nu_c * v) for v in c.B]    # mode 2: nu itself, whatever the op
    yield c
    c.M.close()


def convolve_with_nu(lsfc, M, b):
    """lsfc_convolve(apply_nu = 1) on a host vector"""
    L = lsfc._lib
    y = np.empty_like(b)
    L.check(L.load().lsfc_convolve(M._plan, b.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), 1, L.LSFC_MEM_HOST))
    return y


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("nrhs", [1, 3, 8, 11])
def test_batches(lsfc, small, nrhs, fuse):
    import torch
    c = small
    c.M.set_tuning(batch_fuse=fuse)
    try:
        if nrhs > 1 and c.pruned:
            expect(parse(c.M.describe_passes(min(nrhs, 8)))["store"], batch="fused" if fuse else "per_member")
        for w in ALL + ("G nu",):
            V, mode = (c.M, 2) if w == "G nu" else (view(c.M, w), 0)
            Bd = torch.from_numpy(c.B[:nrhs].copy()).cuda()
            Y = lsfc.apply_batch(V, Bd, mode).cpu().numpy()
            Yh = lsfc.apply_batch(V, c.B[:nrhs], mode)           # host vectors: the same groups through the staging buffers
            assert np.array_equal(Y, Yh), (w, nrhs, fuse)
            for j in range(nrhs):
                judge(Y[j], c.wantB[w][j], c.e_refc if w == "G nu" else c.e_ref, f"batch {w} nrhs={nrhs} fuse={fuse} member {j}")
                if not fuse:
                    single = convolve_with_nu(lsfc, c.M, c.B[j].copy()) if w == "G nu" else (V * torch.from_numpy(c.B[j].copy()).cuda()).cpu().numpy()
                    assert np.array_equal(Y[j], single), (w, nrhs, j)
            assert get_op(lsfc, c.M) == 0 and c.M.nu_is_complex
    finally:
        c.M.set_tuning(batch_fuse=-1)


# ---------------------------------------------------------------------------- 4. host vectors
def test_host_vectors_small_path(lsfc, small):
    import torch
    c = small
    for w in ALL:
        V = view(c.M, w)
        y = V * c.b
        judge(y, c.cwant[w], c.e_ref, f"host small {w}")
        yd = (V * torch.from_numpy(c.b).cuda()).cpu().numpy()
        assert np.array_equal(y, yd), w
        z = c.b.copy()
        V.mul_(z, z)                                             # in place on the host
        assert np.array_equal(z, y), w


@pytest.mark.parametrize("K", ["2", "5"])
def test_host_vectors_chunked_pipeline(lsfc, K, monkeypatch):
    import torch
    c = CSym(lsfc, (48, 40, 80), (24, 20, 40), seed=5).go_complex()
    assert c.M.pipeline == "pruned-hip"
    dev = {}
    for w in ALL:                                                # device-resident results first, no pipeline involved
        dev[w] = (view(c.M, w) * torch.from_numpy(c.b).cuda()).cpu().numpy()
        judge(dev[w], c.cwant[w], c.e_ref, f"device {w}")
    monkeypatch.setenv("LSFC_HOST_PIPELINE", K)
    for w in ALL:                                                # slabs with z0 != 0 read their part of both planes of nu
        V = view(c.M, w)
        y = V * c.b
        assert np.array_equal(y, dev[w]), (K, w)
        z = c.b.copy()
        V.mul_(z, z)
        assert np.array_equal(z, dev[w]), (K, w)
        Y = lsfc.apply_batch(V, np.stack([c.b, c.b.conj(), c.b]), 0)      # two staging slots
        assert np.array_equal(Y[0], dev[w]) and np.array_equal(Y[2], dev[w]), (K, w)
        judge(Y[1], c.cref.of(w)(c.b.conj()), c.e_ref, f"chunked K={K} {w} rhs1")
    c.M.close()


# ---------------------------------------------------------------------------- 5. the dot test, no oracle
def test_dot_test_builder_48(lsfc):
    import torch
    n = 48
    x, h = cases.grid(n, False)
    X, Y, Z = o.grid3d(x, x, x)
    re, im = cases.nu_synthetic(3), cases.nu_synthetic(3, seed=4321)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, 10.0, lambda *c: re(*c) + (2j / 3) * im(*c))
    assert M.pipeline == "pruned-hip" and M.nu_is_complex and np.abs(M.nu.imag).max() > 0.05
    g = torch.Generator(device="cuda").manual_seed(3)
    u = torch.randn(n ** 3, dtype=torch.complex128, device="cuda", generator=g)
    v = torch.randn(n ** 3, dtype=torch.complex128, device="cuda", generator=g)
    Mu = M * u
    scale = float(torch.linalg.norm(Mu) * torch.linalg.norm(v))
    dH = abs(complex(torch.vdot(v, Mu) - torch.vdot(M.H * v, u))) / scale            # <Mu, v> = <u, M^H v>
    dT = abs(complex(torch.sum(Mu * v) - torch.sum(u * (M.T * v)))) / scale          # the bilinear form for M^T
    # (the imaginary part matters at this size: conj(M.T conj v) with nu instead of conj(nu) fails the test by orders of magnitude)
    wrong = abs(complex(torch.vdot(v, Mu) - torch.vdot(torch.conj(M.T * v), u))) / scale
    print(f"dot test 48^3, complex nu: H {dH:.3e}  T {dT:.3e}  (M.T taken for M.H: {wrong:.3e})")
    assert dH < 1e-12 and dT < 1e-12
    assert wrong > 1e-6
    M.close()


# ---------------------------------------------------------------------------- 6. state
def test_nu_state(lsfc, small):
    import torch
    c = small
    L = lsfc._lib
    y_c = {w: view(c.M, w) * c.b for w in ALL}
    # real -> complex -> real: the bits of the plan before it saw a complex nu, and of a fresh real plan
    c.M.set_nu(c.nu)
    assert not c.M.nu_is_complex and c.M.nu.dtype == np.float64
    fresh = c.plan(0)
    assert not fresh.nu_is_complex and fresh.pipeline == c.M.pipeline
    for w in ALL:
        y = view(c.M, w) * c.b
        assert np.array_equal(y, c.y_real[w]) and np.array_equal(y, view(fresh, w) * c.b), w
    fresh.close()
    # a complex dtype with zero imaginary part takes the complex path and agrees with the real one within TOL
    c.M.set_nu(c.nu.astype(np.complex128))
    assert c.M.nu_is_complex
    for w in ALL:
        err = rel_err(view(c.M, w) * c.b, c.y_real[w])
        print(f"zero imaginary part, {w}: {err:.3e} from the real path")
        assert err < TOL
    # from a device tensor: the bits of the host memspace
    c.M.set_nu(c.nu)
    c.M.set_nu(torch.from_numpy(c.nu_c).cuda())
    assert c.M.nu_is_complex and c.M.nu.dtype == np.complex128
    for w in ALL:
        assert np.array_equal(view(c.M, w) * c.b, y_c[w]), w
    flag = C.c_int(-1)
    L.check(L.load().lsfc_plan_nu_is_complex(c.M._plan, C.byref(flag)))
    assert flag.value == 1
    c.M.set_nu(c.nu_c)                                           # (as the fixture left it)
    for w in ALL:
        assert np.array_equal(view(c.M, w) * c.b, y_c[w]), w


def test_profile_bytes(lsfc, small):
    import torch
    c = small
    xd = torch.from_numpy(c.b).cuda()
    yd = torch.empty_like(xd)
    first, last = ("xfwd", "xinv") if c.pruned else ("embed", "crop_axpy")
    pc = {w: {k: b for k, _, b in lsfc.profile_apply(view(c.M, w), xd, yd, 1)} for w in ALL}
    c.M.set_nu(c.nu)
    try:
        pr = {w: {k: b for k, _, b in lsfc.profile_apply(view(c.M, w), xd, yd, 1)} for w in ALL}
    finally:
        c.M.set_nu(c.nu_c)
    for w in ALL:
        stage = first if w == "N" else last
        for k in pr[w]:
            assert pc[w][k] - pr[w][k] == (8 * c.N if k == stage else 0), (w, k)
    # profile_apply ran the op and the nu it was given: the last result in yd is that of H with the complex nu
    lsfc.profile_apply(c.M.H, xd, yd, 1)
    assert np.array_equal(yd.cpu().numpy(), c.M.H * c.b)
    lsfc.time_apply(c.M.T, xd, yd, 2)
    assert np.array_equal(yd.cpu().numpy(), c.M.T * c.b)


def test_state_is_restored(lsfc, small):
    import torch
    c = small
    y0 = {w: view(c.M, w) * c.b for w in ALL}
    xd = torch.from_numpy(c.b).cuda()
    yd = torch.empty_like(xd)
    for w in ALL:
        V = view(c.M, w)
        calls = [lambda: V * c.b, lambda: lsfc.mul_(np.empty(c.N, complex), V, c.b), lambda: lsfc.apply_batch(V, c.B[:2], 0),
                 lambda: lsfc.apply_batch(c.M, c.B[:2], 2), lambda: convolve_with_nu(lsfc, c.M, c.b.copy()),
                 lambda: lsfc.time_apply(V, xd, yd, 1), lambda: lsfc.profile_apply(V, xd, yd, 1),
                 lambda: lsfc.sampleG3D(c.omega, None, None, None, [0, c.N - 1], c.M),
                 lambda: lsfc.gmres_(np.zeros(c.N, complex), V, c.b, restart=5, maxiter=3),
                 lambda: lsfc.gmres_batch_(np.zeros((2, c.N), complex), V, c.B[:2], restart=5, maxiter=3),
                 lambda: lsfc.bicgstabl_(np.zeros(c.N, complex), V, c.b, l=2, max_mv_products=8),
                 lambda: lsfc.bicgstabl_batch_(np.zeros((2, c.N), complex), V, c.B[:2], l=2, max_mv_products=8)]
        for i, f in enumerate(calls):
            f()
            assert get_op(lsfc, c.M) == 0 and c.M.nu_is_complex, (w, i)
        for v in ALL:
            assert np.array_equal(view(c.M, v) * c.b, y0[v]), (w, v)
    # lsfc_sample_sources describes G: rows of the bare Green's matrix, nu nowhere
    rows = lsfc.sampleG3D(c.omega, None, None, None, [5], c.M)
    e = np.zeros(c.N, complex)
    e[5] = 1.0
    judge(rows[0], c.cref.conv(e), c.e_refc, "sample_sources row 5")


# ---------------------------------------------------------------------------- 7. sparsify
SPARSE = [("trap", (21, 21, 1)), ("gv3", (18, 12, 10))]


def special_nu(rng, N):
    nu = rng.uniform(-0.3, 0.3, N) + 1j * complex_part(rng, N)
    nu[::5] = 0.0
    nu[2::9] = 1j * nu[2::9].imag
    return nu


@pytest.mark.parametrize("kind,dims", SPARSE)
def test_sparsify_msp_is_as_plus_k2_ag_nu(lsfc, kind, dims):
    M, _, _, k, _ = gsp.case(kind, dims)
    assert not M.nu_is_complex and M.omega == k
    real = lsfc.sparsify_arrays(M)
    nu = special_nu(np.random.default_rng(sum(dims)), M.N)
    M.set_nu(nu)
    d = lsfc.sparsify_arrays(M)
    for name in ("rowptr", "col", "As", "AG", "sigma"):
        assert np.array_equal(d[name], real[name]), name
    # entry by entry: one complex multiply-add is a handful of roundings of its terms
    want = d["As"] + k ** 2 * d["AG"] * nu[d["col"]]
    bound = 16 * 2.0 ** -53 * (np.abs(d["As"]) + k ** 2 * np.abs(d["AG"]) * np.abs(nu[d["col"]]))
    diff = np.abs(d["Msp"] - want)
    print(f"{kind} {dims}: max |Msp - (As + k^2 AG nu)| / bound = {np.max(diff[bound > 0] / bound[bound > 0]):.3f}")
    assert np.all(diff <= bound)
    # and the imaginary part is there: far from the real-nu Msp
    assert np.abs(d["Msp"] - real["Msp"]).max() > 1e-3 * np.abs(real["Msp"]).max()
    # the pair of the Python front end is this Msp
    Msp, As = lsfc.sparsifying_pair(M)
    assert np.array_equal(gsp._csr(Msp).data, d["Msp"]) and np.array_equal(gsp._csr(As).data, d["As"])
    M.close()


# ---------------------------------------------------------------------------- 8. the preconditioner, 9. the solvers
PHYS = [("trap", (41, 41, 1)), ("gv3", (16, 16, 16))]
BOUND = {("trap", (41, 41, 1)): 5, ("gv3", (16, 16, 16)): 4}    # the oracle's preconditioned GMRES: 4 (against 8-9) and 3 (against 5), + 1
_PHYS = {}


def physical(lsfc, kind, dims, sign):
    """(operator with nu (1 + sign 0.5i), preconditioner from its plan, right-hand side, reference operator, restatement's
    (Msp, As)), once per session; the restatement's rows are assembled once per case"""
    key = (kind, dims)
    if key + (sign,) in _PHYS:
        return _PHYS[key + (sign,)]
    if key not in _PHYS:
        M, rows, nu, k, Mo = gsp.case(kind, dims)
        M.close()
        _PHYS[key] = dict(parts=sref.build(rows, *dims), nu=np.asarray(nu, dtype=np.float64).reshape(-1, order="F"), k=k, Mo=Mo)
    S = _PHYS[key]
    nu_c = S["nu"] * (1 + sign * 0.5j)
    n = dims[0]
    h = 1.0 / n if kind == "gv3" else 1.0 / (n - 1)
    x = -0.5 + h * np.arange(n)
    if kind == "gv3":
        X, Y, Z = o.grid3d(x, x, x)
        M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, S["k"], lambda *c: gsp.nu3(*c) * (1 + sign * 0.5j))
    else:
        X = o.grid2d(x, x)[0]
        M = lsfc.buildFastConvolution(x, x, h, S["k"], lambda *c: gsp.nu2(*c) * (1 + sign * 0.5j), quadRule="trapezoidal")
    assert M.nu_is_complex and rel_err(M.nu, nu_c) < 1e-15
    nu_c = M.nu.copy()
    ref = cr.ref_of_oracle(S["Mo"], nu_c)
    u_inc = np.exp(1j * S["k"] * X).ravel(order="F")
    rhs = -(ref.N(u_inc) - u_inc)                                # examples/example3D.jl:71-72
    _PHYS[key + (sign,)] = M, lsfc.SparsifyingPreconditioner.from_operator(M), rhs, ref, (cr.msp_ref(S["parts"], nu_c, S["k"]), S["parts"]["As"])
    return _PHYS[key + (sign,)]


def elementwise(x, want):
    return bc.elementwise_err(x, want)


@pytest.mark.parametrize("sign", [-1, 1], ids=["absorbing", "amplifying"])
@pytest.mark.parametrize("kind,dims", PHYS)
def test_preconditioner_from_operator(lsfc, kind, dims, sign):
    import scipy.sparse.linalg as spla
    M, P, rhs, ref, (Msp_ref, As_ref) = physical(lsfc, kind, dims, sign)
    b = o.random_vector(M.N)
    err = rel_err(P.solve(b), spla.splu(Msp_ref.tocsc()).solve(As_ref @ b))
    print(f"{kind} {dims} sign {sign:+d}: P.solve against the restatement {err:.3e}")
    assert err <= 1e-9
    # P.T / P.H against scipy on the pair the device itself assembled
    Msp, As = lsfc.sparsifying_pair(M)
    luT = spla.splu(Msp.T.tocsc())
    PT = lambda v: As.T @ luT.solve(v)                           # noqa: E731
    eT, eH = rel_err(P.T.solve(b), PT(b)), rel_err(P.H.solve(b), np.conj(PT(np.conj(b))))
    print(f"{kind} {dims} sign {sign:+d}: P.T {eT:.3e}  P.H {eH:.3e} against scipy on the device's pair")
    assert eT <= 1e-10 and eH <= 1e-10
    # the constructor's two routes on the complex pair the device assembled: host LU with the device's triangular solves, and the
    # block-tridiagonal factorisation with the slowest axis as block index (bars of the from_operator object above)
    want = spla.splu(Msp.tocsc()).solve(As @ b)
    host = lsfc.SparsifyingPreconditioner(Msp, As)
    tri = lsfc.SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=dims[2] if dims[2] > 1 else dims[1])
    try:
        assert np.abs(Msp.data.imag).max() > 0 and np.abs((Msp - As).data.imag).max() > 0
        e_host, e_tri = rel_err(host.solve(b), want), rel_err(tri.solve(b), want)
        print(f"{kind} {dims} sign {sign:+d}: constructor routes against scipy: host LU {e_host:.3e}, blocktri {e_tri:.3e}")
        assert e_host <= 1e-9 and e_tri <= 1e-9
        assert rel_err(tri.T.solve(b), PT(b)) <= 1e-10 and rel_err(tri.H.solve(b), np.conj(PT(np.conj(b)))) <= 1e-10
    finally:
        host.close()
        tri.close()
    # a group of 8 is its singles (bound of tests/test_gpu_precond_transpose.py: 1e-10 in norm and elementwise)
    B8 = bc.right_hand_sides(M.N, 8)
    for Q in (P, P.T, P.H):
        V = Q.solve_batch(B8)
        for j in range(8):
            single = Q.solve(B8[j])
            assert rel_err(V[j], single) <= 1e-10 and elementwise(V[j], single) <= 1e-10, j


@pytest.mark.parametrize("sign", [-1, 1], ids=["absorbing", "amplifying"])
@pytest.mark.parametrize("kind,dims", PHYS)
def test_preconditioned_gmres(lsfc, kind, dims, sign):
    import scipy.sparse.linalg as spla
    M, P, rhs, ref, (Msp_ref, As_ref) = physical(lsfc, kind, dims, sign)
    u, hist = lsfc.gmres_(np.zeros(M.N, complex), M, rhs, Pl=P, reltol=1e-6, log=True)
    u0, hist0 = lsfc.gmres_(np.zeros(M.N, complex), M, rhs, reltol=1e-6, maxiter=400, log=True)
    print(f"{kind} {dims} sign {sign:+d}: {hist.iters} preconditioned steps, {hist0.iters} without")
    assert hist.isconverged and hist.iters <= BOUND[(kind, dims)] and hist.iters < hist0.iters, (hist.iters, hist0.iters)
    lu = spla.splu(Msp_ref.tocsc())
    uo, ho = o.gmres(np.zeros(M.N, complex), ref.N, rhs, Pl=lambda v: lu.solve(As_ref @ v), reltol=1e-6)
    print(f"    the oracle's GMRES with the restatement's preconditioner: {ho.iters} steps; x error {rel_err(u, uo):.3e}")
    assert rel_err(u, uo) <= 1e-8
    # the adjoint system with P.H, GMRES and BiCGStab(l)
    uh, hh = lsfc.gmres_(np.zeros(M.N, complex), M.H, rhs, Pl=P.H, reltol=1e-6, restart=20, log=True)
    res = float(np.linalg.norm(ref.H(uh) - rhs) / np.linalg.norm(rhs))
    ub, hb = lsfc.bicgstabl_(np.zeros(M.N, complex), M.H, rhs, Pl=P.H, reltol=1e-6, log=True)
    resb = float(np.linalg.norm(ref.H(ub) - rhs) / np.linalg.norm(rhs))
    print(f"    M.H with P.H: gmres {hh.iters} steps, true residual {res:.2e}; bicgstabl {hb.mvps} applies, {resb:.2e}")
    assert hh.isconverged and hb.isconverged and res <= 1e-5 and resb <= 1e-5
    assert get_op(lsfc, M) == 0 and M.nu_is_complex


def complex_solver_setup(lsfc, name, flags=0):
    """solver_setup of tests/test_gpu_adjoint.py with nu (1 - 0.5i)"""
    M, _, _, Mo = solver_setup(lsfc, name, flags)
    Cx = cbuilt(name)
    M.set_nu(Cx["nu"])
    c = built(name)["c"]
    X = c["X"] if name == "gv16k10" else o.grid2d(c["x"], c["x"])[0]
    u_inc = cases.plane_wave(c["k"], X)
    rhs = -(Cx["ref"].N(u_inc) - u_inc)
    return M, Cx["ref"], rhs


def check_gmres(u, hist, uo, ho, A, rhs, what):
    """the bounds of check_gmres of tests/test_gpu_adjoint.py"""
    r, ref = np.asarray(hist["resnorm"]), np.asarray(ho.resnorm)
    k = min(len(r), len(ref))
    big = ref[:k] > 1e-6 * ref[0]
    dev = float(np.max((np.abs(r[:k] - ref[:k]) / ref[:k])[big]))
    res = float(np.linalg.norm(A(u) - rhs) / np.linalg.norm(rhs))
    print(f"{what}: iters {hist.iters} (reference {ho.iters}), history deviation {dev:.2e}, x error {rel_err(u, uo):.2e}, true residual {res:.2e}")
    assert hist.isconverged and ho.isconverged
    assert abs(hist.iters - ho.iters) <= 1
    assert dev < 1e-6
    assert rel_err(u, uo) < 1e-7
    assert res < 1e-7


@pytest.mark.parametrize("which", ["T", "H"])
@pytest.mark.parametrize("name", ["gv16k10", "gv32"])
def test_gmres_on_views(lsfc, name, which):
    M, ref, rhs = complex_solver_setup(lsfc, name)
    A = ref.of(which)
    u, hist = lsfc.gmres_(np.zeros(M.N, complex), view(M, which), rhs, restart=20, reltol=1e-8, log=True)
    uo, ho = o.gmres(np.zeros(M.N, complex), A, rhs, restart=20, reltol=1e-8)
    check_gmres(u, hist, uo, ho, A, rhs, f"gmres {name} {which}, complex nu")
    assert get_op(lsfc, M) == 0 and M.nu_is_complex
    M.close()


@pytest.mark.parametrize("name", ["gv16k10", "gv32"])
def test_bicgstabl_on_the_adjoint(lsfc, name):
    M, ref, rhs = complex_solver_setup(lsfc, name)
    A = ref.H
    want = br.bicgstabl_ref(rhs, a=A, pl=None, l=2, reltol=1e-10, dtype=np.complex128)
    res_ref = float(np.linalg.norm(A(want["x"]) - rhs) / np.linalg.norm(rhs))
    u, h = lsfc.bicgstabl_(np.zeros(M.N, complex), M.H, rhs, l=2, reltol=1e-10, log=True)
    res = float(np.linalg.norm(A(u) - rhs) / np.linalg.norm(rhs))
    print(f"bicgstabl {name} H, complex nu: device {h.iters} cycles, true residual {res:.3e}; fp64 restatement {want['iters']} cycles, {res_ref:.3e}")
    assert want["converged"] and h.isconverged
    assert res <= 10 * res_ref
    assert abs(h.iters - want["iters"]) <= 1
    M.close()


@pytest.mark.parametrize("name", ["gv16k10", "gv32"])
def test_batched_solvers_on_the_adjoint_are_their_single_solves(lsfc, name):
    M, ref, rhs = complex_solver_setup(lsfc, name, FORCE_ROCFFT)
    assert M.pipeline == "rocfft-reduced"
    Bm = np.stack([rhs, 1j * rhs[::-1].copy()])
    X, hs = lsfc.gmres_batch_(np.zeros_like(Bm), M.H, Bm, restart=20, reltol=1e-8, log=True)
    for j in range(2):
        x1, h1 = lsfc.gmres_(np.zeros(M.N, complex), M.H, Bm[j], restart=20, reltol=1e-8, log=True)
        kc._bitwise(f"gmres_batch {name}", X, hs, j, x1, h1)
        assert h1.isconverged
    assert float(np.linalg.norm(ref.H(X[0]) - rhs) / np.linalg.norm(rhs)) < 1e-7
    X, hs = lsfc.bicgstabl_batch_(np.zeros_like(Bm), M.H, Bm, l=2, reltol=1e-8, log=True)
    for j in range(2):
        x1, h1 = lsfc.bicgstabl_(np.zeros(M.N, complex), M.H, Bm[j], l=2, reltol=1e-8, log=True)
        kc._bitwise(f"bicgstabl_batch {name}", X, hs, j, x1, h1)
        assert h1.isconverged
    assert float(np.linalg.norm(ref.H(X[0]) - rhs) / np.linalg.norm(rhs)) < 1e-7
    assert get_op(lsfc, M) == 0 and M.nu_is_complex
    M.close()


# ---------------------------------------------------------------------------- 10. refusals
def test_distributed_plans_are_refused(lsfc):
    L = lsfc._lib
    n = 16
    N = n * n * (n // 2)
    rng = np.random.default_rng(3)
    nu = rng.uniform(-0.3, 0.3, N)
    nu_c = nu + 1j * complex_part(rng, N)
    sim = C.c_void_p()
    L.check(L.load().lsfc_dist_sim_plan_create_gv3d(C.byref(sim), n, n, n, 1.0, 3.0, nu.ctypes.data_as(C.c_void_p), 0, 0, 0, 2))
    try:
        flag = C.c_int(-1)
        for memspace in (L.LSFC_MEM_HOST, L.LSFC_MEM_DEVICE):
            assert L.load().lsfc_plan_set_nu_complex(sim, nu_c.ctypes.data_as(C.c_void_p), memspace) == L.LSFC_EINVAL
            assert "complex nu" in L.load().lsfc_last_error().decode()
            assert L.load().lsfc_plan_nu_is_complex(sim, C.byref(flag)) == 0 and flag.value == 0
        # the plan keeps working with its real nu
        assert L.load().lsfc_plan_set_nu(sim, nu.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST) == 0
        assert L.load().lsfc_plan_nu_is_complex(sim, C.byref(flag)) == 0 and flag.value == 0
    finally:
        L.load().lsfc_plan_destroy(sim)
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D, SimulatedRanks
    full = np.concatenate([nu, nu])
    with pytest.raises(TypeError, match="complex nu"):
        SimulatedRanks(n, n, n, 1.0 / n, 3.0, full.astype(np.complex128), 2)
    with pytest.raises(TypeError, match="complex nu"):
        MultiDeviceFastM3D(n, 1.0 / n, 3.0, full.astype(np.complex128), devices=[0, 0])
    S = SimulatedRanks(n, n, n, 1.0 / n, 3.0, full, 2)
    b = o.random_vector(2 * N)
    y0 = S.apply(b)
    for r in range(2):
        assert L.load().lsfc_plan_set_nu_complex(S.plans[r], np.concatenate([nu_c, nu_c]).ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST) == L.LSFC_EINVAL
        assert "complex nu" in L.load().lsfc_last_error().decode()
    assert np.array_equal(S.apply(b), y0)
    S.close()
