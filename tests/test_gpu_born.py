"""GPU tests of linearised scattering (lsfc_born_*, csrc/born.hip, born.py): the two kernel entries against a numpy.longdouble
reference with the rounding bounds of their arithmetic, the bitwise properties of the image sum, and B.data, B * dnu, B.H * r and
misfit against the dense reference of tests/born_ref.py at relative l2 <= 1e-10, the project's parity bound, with the solves at
reltol = 1e-13 (cond(M) <= 10 on every case: tests/test_born_ref_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import born_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-10
U53 = 2.0 ** -53


def _lib():
    import fast_solver_lippmann_schwinger_amd._lib as L
    return L, L.load()


# ---- the kernel entries ------------------------------------------------------------------------------------------------------

DIMS = {216: (6, 6, 6), 630: (10, 9, 7), 4096: (16, 16, 16)}


def literal_operator(lsfc, dims, k, nu):
    """FastM3D on a grid with odd axes, which buildFastConvolution3D does not take: the truncated kernel of the reference
    (src/Functions.jl:49-51) on the lattice 2 pi / (4 h n_a) of each axis, truncation radius 1.8 x the longest side.  The symbol
    depends on |s| alone, so the Green's matrix is symmetric."""
    from oracle import lsfc_oracle as o
    h = 1.0 / dims[0]
    f = [2.0 * np.pi / (4.0 * h * d) * np.arange(-2 * d, 2 * d, dtype=np.float64) for d in dims]
    S = np.sqrt(f[0][:, None, None] ** 2 + f[1][None, :, None] ** 2 + f[2][None, None, :] ** 2)
    G = o.gtruncated3d(1.8 * h * max(dims), float(k), S, True)
    return lsfc.FastM3D(G, nu, 4 * dims[0], 4 * dims[1], 4 * dims[2], dims[0], dims[1], dims[2], k)


@functools.lru_cache(maxsize=None)
def plan_of(N):
    """a plan with N grid points: the kernel entries take N, device and stream from it and nothing else"""
    import fast_solver_lippmann_schwinger_amd as lsfc
    dims = DIMS[N]
    if any(d % 2 for d in dims):
        return literal_operator(lsfc, dims, 2.0, np.zeros(N))
    ax, h = ref.axes_of(dims)
    return lsfc.buildFastConvolution3D(*ax, *ref.coords_of(dims), h, 2.0, np.zeros(N))


def ld(z):
    return z.real.astype(np.longdouble), z.imag.astype(np.longdouble)


def cmul_ld(a, b):
    (ar, ai), (br, bi) = ld(np.asarray(a, dtype=complex)), ld(np.asarray(b, dtype=complex))
    return ar * br - ai * bi, ar * bi + ai * br


def run_scale(N, dnu, Umat, device, alias):
    L, lib = _lib()
    M = plan_of(N)
    nrhs = Umat.shape[0]
    is_c = int(np.iscomplexobj(dnu))
    if device:
        import torch
        d, u = torch.from_numpy(np.ascontiguousarray(dnu)).cuda(), torch.from_numpy(Umat.copy()).cuda()
        out = u if alias else torch.empty_like(u)
        L.check(lib.lsfc_born_scale(M._plan, C.c_void_p(d.data_ptr()), is_c, C.c_void_p(u.data_ptr()), C.c_void_p(out.data_ptr()), nrhs, L.LSFC_MEM_DEVICE))
        M.synchronize()
        if not alias:
            assert np.array_equal(u.cpu().numpy(), Umat)
        return out.cpu().numpy()
    d, u = np.ascontiguousarray(dnu), Umat.copy()
    out = u if alias else np.empty_like(u)
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    L.check(lib.lsfc_born_scale(M._plan, p(d), is_c, p(u), p(out), nrhs, L.LSFC_MEM_HOST))
    return out


def run_image(N, Umat, Pmat, scale, flags, g=None, device=False):
    L, lib = _lib()
    M = plan_of(N)
    nrhs = Umat.shape[0]
    real = bool(flags & L.LSFC_BORN_REAL)
    if g is None:
        g = np.full(N, np.nan, dtype=np.float64 if real else np.complex128)      # without ACCUMULATE what g held is not read
    g = g.copy()
    if device:
        import torch
        u, p_, gd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Umat, Pmat, g))
        L.check(lib.lsfc_born_image(M._plan, C.c_void_p(u.data_ptr()), C.c_void_p(p_.data_ptr()), nrhs, scale.real, scale.imag, flags,
                                    C.c_void_p(gd.data_ptr()), L.LSFC_MEM_DEVICE))
        M.synchronize()
        return gd.cpu().numpy()
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)             # noqa: E731
    Uc, Pc = np.ascontiguousarray(Umat), np.ascontiguousarray(Pmat)
    L.check(lib.lsfc_born_image(M._plan, p(Uc), p(Pc), nrhs, scale.real, scale.imag, flags, g.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
    return g


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("N", list(DIMS))
def test_scale_against_longdouble(N, device):
    rng = np.random.default_rng(N)
    for nrhs in (1, 7, 8, 9, 17):
        Umat = ref.cvec(rng, nrhs, N)
        for dnu in (rng.standard_normal(N), ref.cvec(rng, N)):
            wr, wi = cmul_ld(dnu[None, :], Umat)
            bound = 4 * U53 * np.abs(dnu)[None, :] * np.abs(Umat)
            for alias in (False, True):
                got = run_scale(N, dnu, Umat, device, alias)
                err = np.hypot((got.real - wr).astype(float), (got.imag - wi).astype(float))
                worst = float((err / bound).max())
                print(f"  scale N {N} nrhs {nrhs} complex {np.iscomplexobj(dnu)} alias {alias}: max err / bound {worst:.3f}")
                assert worst <= 1.0


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("N", list(DIMS))
def test_image_against_longdouble(N, device):
    L, _ = _lib()
    rng = np.random.default_rng(N + 1)
    scale = complex(-2.25, 0.75)
    for nrhs in (1, 7, 8, 9, 17):
        Umat, Pmat = ref.cvec(rng, nrhs, N), ref.cvec(rng, nrhs, N)
        tr, ti = cmul_ld(Umat, Pmat)
        sr, si = np.longdouble(scale.real), np.longdouble(scale.imag)
        wr, wi = (sr * tr + si * ti).sum(axis=0), (si * tr - sr * ti).sum(axis=0)          # scale * conj(t)
        bound = (nrhs + 6) * 2 * U53 * abs(scale) * (np.abs(Umat) * np.abs(Pmat)).sum(axis=0)
        got = run_image(N, Umat, Pmat, scale, 0, device=device)
        err = np.hypot((got.real - wr).astype(float), (got.imag - wi).astype(float))
        worst = float((err / bound).max())
        print(f"  image N {N} nrhs {nrhs}: max err / bound {worst:.3f}")
        assert worst <= 1.0
        re = run_image(N, Umat, Pmat, scale, L.LSFC_BORN_REAL, device=device)
        assert re.dtype == np.float64 and np.array_equal(re, got.real)


@pytest.mark.parametrize("N", [216, 630])
def test_image_bits(N):
    L, _ = _lib()
    ACC, REAL = L.LSFC_BORN_ACCUMULATE, L.LSFC_BORN_REAL
    rng = np.random.default_rng(5)
    Umat, Pmat = ref.cvec(rng, 17, N), ref.cvec(rng, 17, N)
    scale = complex(-9.0, 0.5)
    for flags in (0, REAL):
        one = run_image(N, Umat, Pmat, scale, flags)
        assert np.array_equal(one, run_image(N, Umat, Pmat, scale, flags)), "two runs"
        assert np.array_equal(one, run_image(N, Umat, Pmat, scale, flags, device=True)), "host and device vectors"
        g = run_image(N, Umat[:8], Pmat[:8], scale, flags)
        g = run_image(N, Umat[8:16], Pmat[8:16], scale, flags | ACC, g=g)
        g = run_image(N, Umat[16:], Pmat[16:], scale, flags | ACC, g=g)
        assert np.array_equal(one, g), "8 + 8 + 1"
        g = run_image(N, Umat[:1], Pmat[:1], scale, flags)
        for j in range(1, 17):
            g = run_image(N, Umat[j:j + 1], Pmat[j:j + 1], scale, flags | ACC, g=g)
        assert np.array_equal(one, g), "17 calls of one"
    assert np.array_equal(run_image(N, Umat, Pmat, scale, REAL), run_image(N, Umat, Pmat, scale, 0).real)
    # the order of the members is what the bits depend on
    assert not np.array_equal(run_image(N, Umat[::-1], Pmat[::-1], scale, 0), run_image(N, Umat, Pmat, scale, 0))


# ---- the object against the dense reference ----------------------------------------------------------------------------------

# the cases of born_ref.CASES take dense G from the oracle; the rectangular one (odd axes: a literal symbol, literal_operator) takes
# it from the library's own convolution of identity columns, which the existing apply tests pin to the oracle
RECT = ref.Case((10, 9, 7), 5.0, 0.3)


def operator_of(lsfc, case, nu):
    ax, h = ref.axes_of(case.dims)
    X = ref.coords_of(case.dims)
    if len(case.dims) == 2:
        M = lsfc.buildFastConvolution(ax[0], ax[1], h, case.k, lambda *_: np.real(nu), quadRule="Greengard_Vico")
    elif any(d % 2 for d in case.dims):
        return literal_operator(lsfc, case.dims, case.k, nu)
    else:
        M = lsfc.buildFastConvolution3D(*ax, *X, h, case.k, np.real(nu))
    if np.iscomplexobj(nu):
        M.set_nu(nu)
    return M


_G_RECT = {}


def green(lsfc, name):
    if name != "10x9x7":
        return ref.CASES[name], ref.dense_G(name)
    if name not in _G_RECT:
        N = int(np.prod(RECT.dims))
        M = operator_of(lsfc, RECT, np.zeros(N))
        G = lsfc.apply_batch(M, np.eye(N, dtype=complex), mode=1).T.copy()
        M.close()
        assert np.abs(G - G.T).max() <= 1e-13 * np.abs(G).max()
        assert max(np.linalg.cond(ref.dense_M(G, ref.nu_of(RECT, c), RECT.k)) for c in (False, True)) <= 10.0
        G.setflags(write=False)
        _G_RECT[name] = G
    return RECT, _G_RECT[name]


def receivers_of(lsfc, case, kind, count):
    ax, _ = ref.axes_of(case.dims)
    c = ref.receivers(case, kind, count)
    R = lsfc.Receivers(*ax, k=case.k, **({"points": c} if kind == ref.POINTS else {"directions": c}))
    return R, ref.dense_R(case, kind, c)


def check_object(lsfc, case, G, kind, nsrc, complex_nu, **kw):
    nu = ref.nu_of(case, complex_nu)
    M = operator_of(lsfc, case, nu)
    R, Rd = receivers_of(lsfc, case, kind, 5)
    U_inc = ref.plane_waves(case, nsrc)
    B = lsfc.BornOperator(M, R, U_inc, reltol=1e-13, **kw)
    assert B.converged, B.message
    assert len(B.history) == nsrc and all(h.isconverged for h in B.history)
    k = case.k
    U, d = ref.forward(G, Rd, nu, k, U_inc)
    figures = {"fields": ref.rel(B.fields.cpu().numpy(), U), "data": ref.rel(B.data, d)}
    rng = np.random.default_rng(21)
    for cd in (False, True):
        dnu = ref.perturbation(case, complex_=cd)
        got = B * dnu
        assert got.shape == (nsrc, 5) and B.converged
        figures[f"J complex dnu {cd}"] = ref.rel(got, ref.J(G, Rd, nu, k, U, dnu))
        assert np.array_equal(got, B.apply(dnu)), "two calls, the same bits"
    r = ref.cvec(rng, nsrc, 5)
    g = B.H * r
    figures["JH"] = ref.rel(g, ref.JH(G, Rd, nu, k, U, r))
    assert np.array_equal(B.adjoint(r, real=True), g.real)
    assert np.array_equal(g, B.adjoint(r)), "two calls, the same bits"
    # the dot identity through the library
    dnu = ref.perturbation(case, complex_=True)
    Jd = B * dnu
    defect = abs(np.vdot(r, Jd) - np.vdot(g, dnu)) / (np.linalg.norm(r) * np.linalg.norm(Jd))
    figures["dot"] = defect
    d_obs = ref.forward(G, Rd, 1.2 * nu, k, U_inc)[1]
    phi, grad = B.misfit(d_obs)
    phi_ref, grad_ref = ref.misfit(G, Rd, nu, k, U_inc, d_obs)
    assert grad.dtype == (np.complex128 if complex_nu else np.float64)
    figures["phi"], figures["grad"] = abs(phi - phi_ref) / phi_ref, ref.rel(grad, grad_ref)
    print("  " + ", ".join(f"{n} {v:.1e}" for n, v in figures.items()))
    for name, v in figures.items():
        assert v <= TOL, (name, v)
    chunk = B.info()["chunk"]
    B.close(), R.close(), M.close()
    return chunk


@pytest.mark.parametrize("complex_nu", [False, True])
@pytest.mark.parametrize("kind", [ref.FAR, ref.POINTS])
@pytest.mark.parametrize("name", ["6^3", "8^3-kh0.8", "10x9x7", "10^2"])
def test_parity_on_every_grid(lsfc, name, kind, complex_nu):
    case, G = green(lsfc, name)
    check_object(lsfc, case, G, kind, 3, complex_nu)


@pytest.mark.parametrize("solver", ["gmres", "bicgstabl"])
@pytest.mark.parametrize("chunk", [1, 2, 8, None])
@pytest.mark.parametrize("nsrc", [1, 3, 9])
def test_parity_for_every_chunking_and_solver(lsfc, nsrc, chunk, solver):
    case, G = green(lsfc, "6^3")
    used = check_object(lsfc, case, G, ref.FAR, nsrc, nsrc == 3, chunk=chunk, solver=solver, l=2)
    assert used == (min(chunk, nsrc) if chunk else nsrc)


def test_central_difference_through_the_library(lsfc):
    # J dnu against (d(nu + e dnu) - d(nu - e dnu)) / 2e by two updates: truncation <= 1.1e-8 on the dense reference at e = 1e-4,
    # solver noise 2 * 1e-13 * cond / e ~ 5e-9
    case = ref.CASES["8^3-kh0.8"]
    nu = ref.nu_of(case)
    M = operator_of(lsfc, case, nu)
    R, _ = receivers_of(lsfc, case, ref.FAR, 5)
    B = lsfc.BornOperator(M, R, ref.plane_waves(case, 3), reltol=1e-13)
    dnu = ref.perturbation(case)
    dnu /= np.abs(dnu).max()
    Jd = B * dnu
    e = 1e-4
    B.update(nu + e * dnu)
    dp = B.data
    B.update(nu - e * dnu)
    dm = B.data
    err = ref.rel(Jd, (dp - dm) / (2 * e))
    print(f"  J vs central difference through the library: {err:.2e}")
    assert err <= 1e-6


def ops_of(M, P):
    L, lib = _lib()
    a, b = C.c_int(-1), C.c_int(-1)
    L.check(lib.lsfc_plan_get_op(M._plan, C.byref(a)))
    L.check(lib.lsfc_precond_get_op(P._pc, C.byref(b), None))
    return a.value, b.value


def test_with_the_device_preconditioner(lsfc):
    import sparsify_cases as sc
    L, lib = _lib()
    case = ref.Case((4, 4, 4), 4.0, 0.3)                    # the smallest 3D shape of tests/sparsify_cases.py ("gv3", (4, 4, 4))
    assert sc.find("gv3", case.dims).dims == min((c.dims for c in sc.CASES if c.kind == "gv3"), key=lambda d: int(np.prod(d)))
    ref.CASES["4^3"] = case
    G = ref.dense_G("4^3")
    nu = ref.nu_of(case)
    M = operator_of(lsfc, case, nu)
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    R, Rd = receivers_of(lsfc, case, ref.FAR, 5)
    U_inc = ref.plane_waves(case, 3)
    before = ops_of(M, P)
    assert before == (L.LSFC_OP_N, L.LSFC_OP_N)
    B = lsfc.BornOperator(M, R, U_inc, Pl=P, reltol=1e-13)
    assert ops_of(M, P) == before and B.converged
    U, d = ref.forward(G, Rd, nu, case.k, U_inc)
    assert ref.rel(B.data, d) <= TOL
    dnu = ref.perturbation(case)
    assert ref.rel(B * dnu, ref.J(G, Rd, nu, case.k, U, dnu)) <= TOL and ops_of(M, P) == before
    r = ref.cvec(np.random.default_rng(3), 3, 5)
    assert ref.rel(B.H * r, ref.JH(G, Rd, nu, case.k, U, r)) <= TOL and ops_of(M, P) == before
    sweeps = P.batch_info()["sweeps"]
    assert sweeps > 0                                       # the preconditioner was applied, in group sweeps
    # under another op of plan and preconditioner: the same results, and both are put back to that op
    L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_H))
    L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_H))
    try:
        assert ref.rel(B * dnu, ref.J(G, Rd, nu, case.k, U, dnu)) <= TOL and ops_of(M, P) == (L.LSFC_OP_H, L.LSFC_OP_H)
        assert ref.rel(B.H * r, ref.JH(G, Rd, nu, case.k, U, r)) <= TOL and ops_of(M, P) == (L.LSFC_OP_H, L.LSFC_OP_H)
    finally:
        L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N))
        L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_N))
    B.close()
    # a forced LSFC_ENOTCONV: the outputs are written, the message names source and stage, every source has its result, the ops are back
    # (reltol = 0: on this grid the preconditioner is close to the inverse, and one iteration can reach 1e-13.  restart = 1: GMRES
    # updates x at the end of a cycle, so a longer cycle cut by maxiter = 1 would leave U = 0 and every later right-hand side with it)
    B1 = lsfc.BornOperator(M, R, U_inc, Pl=P, reltol=0.0, restart=1, maxiter=1)
    print("  forced: " + ", ".join(f"{h.iters} its {h.mvps} mvps {h['resnorm'][0]:.1e}" for h in B1.history))
    assert np.abs(B1.fields.cpu().numpy()).min(axis=1).max() > 0
    assert not B1.converged and "source 0" in B1.message and "background solve" in B1.message
    assert len(B1.history) == 3 and not any(h.isconverged for h in B1.history) and ops_of(M, P) == before
    assert np.all(np.isfinite(B1.data))
    out = B1 * dnu
    assert not B1.converged and "solve on M^T" in B1.message and np.all(np.isfinite(out)) and ops_of(M, P) == before
    out = B1.H * r
    assert not B1.converged and "adjoint-state solve" in B1.message and np.all(np.isfinite(out)) and ops_of(M, P) == before
    B1.close()
    # a host-LU object has no transposed apply: accepted for the background and J^H, refused for J with the reason
    Plu = lsfc.SparsifyingPreconditioner(*lsfc.sparsifying_pair(M))
    B2 = lsfc.BornOperator(M, R, U_inc, Pl=Plu, reltol=1e-13)
    assert B2.converged and ref.rel(B2.data, d) <= TOL
    assert ref.rel(B2.H * r, ref.JH(G, Rd, nu, case.k, U, r)) <= TOL
    with pytest.raises(L.LsfcError) as e:
        B2 * dnu
    assert e.value.code == L.LSFC_EINVAL and "cannot follow" in str(e.value) and "block-tridiagonal" in str(e.value)
    a = C.c_int(-1)
    L.check(lib.lsfc_plan_get_op(M._plan, C.byref(a)))
    assert a.value == L.LSFC_OP_N
    B2.close()


def test_refusals_that_need_objects(lsfc):
    L, lib = _lib()
    case = ref.CASES["6^3"]
    M = operator_of(lsfc, case, ref.nu_of(case))
    R, _ = receivers_of(lsfc, case, ref.FAR, 2)
    ax, _h = ref.axes_of(case.dims)
    opts = L.BornOpts(solver=L.LSFC_BORN_GMRES)
    b = C.c_void_p()
    # apply, fields and data before set_background
    L.check(lib.lsfc_born_create(C.byref(b), M._plan, R._rc, C.byref(opts)))
    buf = np.zeros(216, complex)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.lsfc_born_apply(b, p, 1, p, L.LSFC_OP_N, 0, L.LSFC_MEM_HOST) == L.LSFC_EINVAL
    assert "before lsfc_born_set_background" in lib.lsfc_last_error().decode()
    assert lib.lsfc_born_data(b, p, L.LSFC_MEM_HOST) == L.LSFC_EINVAL
    q, n = C.c_void_p(), C.c_int64(0)
    assert lib.lsfc_born_fields(b, C.byref(q), C.byref(n)) == L.LSFC_EINVAL
    assert lib.lsfc_born_destroy(b) == 0
    # receivers of another grid
    R2 = lsfc.Receivers(ax[0][:5], ax[1], ax[2], k=case.k, directions=[[0.0, 0.6, 0.8]])
    assert lib.lsfc_born_create(C.byref(b), M._plan, R2._rc, C.byref(opts)) == L.LSFC_EINVAL
    assert "grid points" in lib.lsfc_last_error().decode() and b.value is None
    # a multi-device plan and a simulated rank
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n16 = 16
    Mm = MultiDeviceFastM3D(n16, 1.0 / n16, 3.0, np.zeros(n16 ** 3), devices=[0, 0])
    try:
        assert lib.lsfc_born_create(C.byref(b), Mm._plan, R._rc, C.byref(opts)) == L.LSFC_EINVAL
        assert "not available on a multi-device plan" in lib.lsfc_last_error().decode()
        assert lib.lsfc_born_scale(Mm._plan, p, 1, p, p, 1, L.LSFC_MEM_HOST) == L.LSFC_EINVAL
        assert lib.lsfc_born_image(Mm._plan, p, p, 1, 1.0, 0.0, 0, p, L.LSFC_MEM_HOST) == L.LSFC_EINVAL
    finally:
        Mm.close()
    sim = C.c_void_p()
    nus = np.zeros(n16 * n16 * (n16 // 2))
    L.check(lib.lsfc_dist_sim_plan_create_gv3d(C.byref(sim), n16, n16, n16, 1.0, 3.0, nus.ctypes.data_as(C.c_void_p), 0, 0, 0, 2))
    try:
        assert lib.lsfc_born_create(C.byref(b), sim, R._rc, C.byref(opts)) == L.LSFC_EINVAL
        assert "not available on a distributed" in lib.lsfc_last_error().decode()
    finally:
        lib.lsfc_plan_destroy(sim)
    # a plan whose Green's matrix is not symmetric: the message of lsfc_plan_set_op
    import sparsify_cases as sc
    Mn = sc.literal_operator(lsfc, (6, 8, 10), "none")
    Rn = lsfc.Receivers(np.arange(6.0), np.arange(8.0), np.arange(10.0), k=2.0, directions=[[0.0, 0.6, 0.8]])
    assert lib.lsfc_born_create(C.byref(b), Mn._plan, Rn._rc, C.byref(opts)) == L.LSFC_EINVAL
    assert "not symmetric" in lib.lsfc_last_error().decode() and b.value is None
    with pytest.raises(NotImplementedError):
        lsfc.BornOperator(M, R, ref.plane_waves(case, 1)).T


def test_lsqr_recovers_a_planted_perturbation(lsfc):
    # kh = 2.7 and a weak medium: 24 sources x 32 directions see every Fourier component of the 6^3 grid (cond(J) = 9.6 on the dense
    # reference), so LSQR converges in about 60 iterations; at kh = 0.5 cond(J) is 1e11 and no iteration recovers anything
    from scipy.sparse.linalg import lsqr
    case = ref.Case((6, 6, 6), 16.0, 0.02)
    nu = ref.nu_of(case)
    M = operator_of(lsfc, case, nu)
    ax, _ = ref.axes_of(case.dims)
    R = lsfc.Receivers(*ax, k=case.k, directions=ref.receivers(case, ref.FAR, 32))
    B = lsfc.BornOperator(M, R, ref.plane_waves(case, 24), reltol=1e-12)
    assert B.shape == (24 * 32, 216) and B.shape[0] >= B.shape[1]
    A = B.aslinearoperator()
    planted = ref.perturbation(case)
    x, istop, itn = lsqr(A, A.matvec(planted.astype(complex)), atol=1e-11, btol=1e-11, conlim=1e12, iter_lim=200)[:3]
    err = ref.rel(x, planted)
    print(f"  lsqr: {itn} iterations, stop {istop}, recovery {err:.2e}")
    assert err <= 1e-8
