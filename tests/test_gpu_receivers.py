"""GPU tests of the off-grid sampling operator (lsfc_receivers_*, csrc/receivers.hip, receivers.py) against the dense numpy /
scipy reference of tests/receivers_ref.py: relative l2 <= 1e-10, the project's parity bound, at the smallest shapes at which the
kernels can go wrong; every phase k r stays below 200.  The bitwise properties of the header are checked as such."""
import ctypes as C
import functools

import numpy as np
import pytest

import receivers_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-10
K = 11.0
POINTS, FAR = 0, 1
# name -> (dims, h, origin): less than a wave; unequal axes; N = 1023 / 1024 (the red_blocks boundary); N = 1025; red_blocks saturated
GRIDS = {
    "3x3x3": ((3, 3, 3), 1.0 / 8, (-0.37, -0.30, -0.21)),
    "6x5x4": ((6, 5, 4), 1.0 / 8, (-0.37, -0.30, -0.21)),
    "31x33": ((31, 33), 1.0 / 8, (-1.37, -2.30)),
    "32x32": ((32, 32), 1.0 / 8, (-1.37, -2.30)),
    "5x5x41": ((5, 5, 41), 1.0 / 8, (-0.37, -0.30, -2.21)),
    "1024x1025": ((1024, 1025), 1.0 / 128, (-3.37, -4.30)),
}


def receiver_points(dims, h, origin, count, seed=3):
    """in turn: 0.07 h from a grid point, outside the box, inside the box between grid points"""
    rng = np.random.default_rng(seed)
    nd = len(dims)
    o, ext = np.array(origin), h * (np.array(dims) - 1)
    pts = np.empty((count, nd))
    for r in range(count):
        u = ref.random_directions(rng, 1, nd)[0]
        idx = np.array([rng.integers(0, d) for d in dims])
        if r % 3 == 0:
            pts[r] = o + h * idx + 0.07 * h * u
        elif r % 3 == 1:
            pts[r] = o + ext / 2 + u * (np.linalg.norm(ext) / 2 + 0.5 + rng.random())
        else:
            pts[r] = o + h * (np.minimum(idx, np.array(dims) - 2).clip(0) + 0.2 + 0.6 * rng.random(nd))
    return pts


def coords_for(kind, dims, h, origin, count, seed=3):
    if kind == FAR:
        return ref.random_directions(np.random.default_rng(seed), count, len(dims))
    return receiver_points(dims, h, origin, count, seed)


def max_phase(kind, grid, c, k=K):
    """the largest k r (points) or k |theta . x| (far field) of the case, from the corners of the box"""
    import itertools
    dims, h, origin = GRIDS[grid]
    corners = np.array([[origin[a] + h * (dims[a] - 1) * bit[a] for a in range(len(dims))] for bit in itertools.product((0, 1), repeat=len(dims))])
    if kind == FAR:
        return k * np.abs(corners @ c.T).max()
    return k * np.sqrt(((c[:, None, :] - corners[None, :, :]) ** 2).sum(axis=2)).max()


def axes_of(dims, h, origin):
    return [origin[a] + h * np.arange(dims[a]) for a in range(len(dims))]


def build(lsfc, grid, kind, count, seed=3, k=K):
    dims, h, origin = GRIDS[grid]
    c = coords_for(kind, dims, h, origin, count, seed)
    R = lsfc.Receivers(*axes_of(dims, h, origin), k=k, **({"points": c} if kind == POINTS else {"directions": c}))
    return R, c


@functools.lru_cache(maxsize=None)
def dense(grid, kind, count, seed=3, k=K):
    dims, h, origin = GRIDS[grid]
    D = ref.dense(kind, dims, origin, h, k, coords_for(kind, dims, h, origin, count, seed))
    D.setflags(write=False)
    return D


def rt_and_chunk(lsfc):
    R, _ = build(lsfc, "3x3x3", FAR, 1)
    i = R.info()
    R.close()
    return i["receivers_per_thread"], i["chunk"]


def check_all_ops(R, D, nrhs, seed, as_torch=False):
    rng = np.random.default_rng(seed)
    Q, W = ref.cvec(rng, nrhs, D.shape[1]), ref.cvec(rng, nrhs, D.shape[0])
    if as_torch:
        import torch
        up, down = (lambda a: torch.from_numpy(a).cuda()), (lambda t: t.cpu().numpy())
    else:
        up = down = lambda a: a
    for op, V, want in (("N", Q, Q @ D.T), ("T", W, W @ D), ("H", W, W @ D.conj())):
        Vin = up(V)
        got = down(R.apply_batch(Vin, op=op))
        assert got.shape == want.shape
        err = ref.rel(got, want)
        print(f"  op {op} nrhs {nrhs}: rel l2 {err:.2e}")
        assert err <= TOL, (op, nrhs, err)
        assert np.array_equal(down(Vin), V)                   # the input is left alone


@pytest.mark.parametrize("kind", [POINTS, FAR])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_parity_on_every_grid(lsfc, grid, kind):
    RT, _ = rt_and_chunk(lsfc)
    count = 2 if grid == "1024x1025" else 2 * RT + 1
    R, c = build(lsfc, grid, kind, count)
    D = dense(grid, kind, count)
    assert R.shape == D.shape and R.info()["N"] == D.shape[1] and R.info()["nrecv"] == count
    assert max_phase(kind, grid, c) < 200
    check_all_ops(R, D, 2, seed=11)


@pytest.mark.parametrize("kind", [POINTS, FAR])
@pytest.mark.parametrize("grid", ["6x5x4", "31x33"])
def test_receiver_counts_around_the_kernel_boundaries(lsfc, grid, kind):
    RT, CH = rt_and_chunk(lsfc)
    assert RT >= 2 and CH >= 2
    dims, h, origin = GRIDS[grid]
    rng = np.random.default_rng(17)
    for count in sorted({1, RT - 1, RT, RT + 1, 2 * RT + 1}):
        R, _ = build(lsfc, grid, kind, count)
        D = dense(grid, kind, count)
        q = ref.cvec(rng, D.shape[1])
        assert ref.rel(R * q, D @ q) <= TOL, ("N", count)
    for count in sorted({1, CH - 1, CH, CH + 1}):
        R, _ = build(lsfc, grid, kind, count)
        D = dense(grid, kind, count)
        w = ref.cvec(rng, count)
        assert ref.rel(R.T * w, D.T @ w) <= TOL, ("T", count)
        assert ref.rel(R.H * w, D.conj().T @ w) <= TOL, ("H", count)


@pytest.mark.parametrize("as_torch", [False, True])
@pytest.mark.parametrize("kind", [POINTS, FAR])
@pytest.mark.parametrize("grid", ["6x5x4", "31x33"])
def test_member_counts_host_and_device(lsfc, grid, kind, as_torch):
    R, _ = build(lsfc, grid, kind, 5)
    D = dense(grid, kind, 5)
    for nrhs in (1, 2, 8, 9):
        check_all_ops(R, D, nrhs, seed=23 + nrhs, as_torch=as_torch)


@pytest.mark.parametrize("kind", [POINTS, FAR])
@pytest.mark.parametrize("grid", ["6x5x4", "32x32", "5x5x41"])
def test_bitwise_properties(lsfc, grid, kind):
    RT, _ = rt_and_chunk(lsfc)
    count, pick = 2 * RT + 1, RT + 1
    R, c = build(lsfc, grid, kind, count)
    dims, h, origin = GRIDS[grid]
    alone = lsfc.Receivers(*axes_of(dims, h, origin), k=K, **({"points": c[pick:pick + 1]} if kind == POINTS else {"directions": c[pick:pick + 1]}))
    rng = np.random.default_rng(29)
    Q, W = ref.cvec(rng, 9, R.N), ref.cvec(rng, 9, count)
    for op, V in (("N", Q), ("T", W), ("H", W)):
        full = R.apply_batch(V, op=op)
        assert np.array_equal(full, R.apply_batch(V, op=op)), (op, "the same call twice")
        for j in (0, 4, 8):                                                   # a member alone, a member among 9
            assert np.array_equal(R.apply(V[j], op=op), full[j]), (op, "member", j)
    # a receiver alone, the same receiver among 2 RT + 1
    assert np.array_equal(alone * Q[0], (R * Q[0])[pick:pick + 1])
    w1 = np.zeros(count, complex)
    w1[pick] = W[0, pick]
    for op in ("T", "H"):
        assert np.array_equal(alone.apply(w1[pick:pick + 1], op=op), R.apply(w1, op=op)), (op, "receiver alone")


@pytest.mark.parametrize("kind", [POINTS, FAR])
@pytest.mark.parametrize("grid", ["6x5x4", "31x33"])
def test_adjoint_identity_on_the_device(lsfc, grid, kind):
    R, _ = build(lsfc, grid, kind, 7)
    rng = np.random.default_rng(31)
    q, w = ref.cvec(rng, R.N), ref.cvec(rng, 7)
    lhs, rhs = np.vdot(w, R * q), np.vdot(R.H * w, q)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    lhs, rhs = np.sum(w * (R * q)), np.sum((R.T * w) * q)                     # the transpose: the bilinear form
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


# ---- the fused forms -------------------------------------------------------------------------------------------------------

def plan8(lsfc, k=6.0):
    n = 8
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    Xg, Yg, Zg = np.meshgrid(x, x, x, indexing="ij")
    X, Y, Z = (A.reshape(-1, order="F") for A in (Xg, Yg, Zg))
    nu = 0.3 * np.exp(-10 * (X ** 2 + Y ** 2 + Z ** 2)) * (1.0 + 0.2 * X)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu)
    return M, x, h, k, nu


@pytest.mark.parametrize("kind", [POINTS, FAR])
def test_fused_medium_real_and_complex(lsfc, kind):
    import fast_solver_lippmann_schwinger_amd._lib as L
    M, x, h, k, nu = plan8(lsfc)
    dims, origin = (8, 8, 8), (x[0], x[0], x[0])
    c = coords_for(kind, dims, h, origin, 6, seed=41)
    R = lsfc.Receivers(x, x, x, k=k, **({"points": c} if kind == POINTS else {"directions": c}))
    D = ref.dense(kind, dims, origin, h, k, c)
    rng = np.random.default_rng(43)
    U, W = ref.cvec(rng, 2, 512), ref.cvec(rng, 2, 6)
    w2 = k * k

    def check(nuv):
        for op, V, want in (("N", U, -w2 * (U * nuv) @ D.T), ("T", W, -w2 * nuv * (W @ D)), ("H", W, -w2 * np.conj(nuv) * (W @ D.conj()))):
            got = R.apply_batch(V, op=op, M=M)
            err = ref.rel(got, want)
            print(f"  fused {op}: rel l2 {err:.2e}")
            assert err <= TOL, (op, err)
        return [R.apply_batch(V, op=op, M=M) for op, V in (("N", U), ("T", W), ("H", W))]

    real_bits = check(nu)
    assert np.array_equal(R.scattered_field(M, U[0]), real_bits[0][0])
    assert np.array_equal(R.adjoint_source(M, W[1]), real_bits[2][1])
    # the plan's op is neither read nor changed, also when it is T
    op = C.c_int(-1)
    L.check(L.load().lsfc_plan_set_op(M._plan, L.LSFC_OP_T))
    try:
        under_t = [R.apply_batch(V, op=o, M=M) for o, V in (("N", U), ("T", W), ("H", W))]
        L.check(L.load().lsfc_plan_get_op(M._plan, C.byref(op)))
        assert op.value == L.LSFC_OP_T
    finally:
        L.check(L.load().lsfc_plan_set_op(M._plan, L.LSFC_OP_N))
    assert all(np.array_equal(a, b) for a, b in zip(under_t, real_bits))
    # a view of M carries the medium of M
    assert np.array_equal(R.scattered_field(M.H, U[0]), real_bits[0][0])
    # complex nu, then back to real: bit for bit the never-complex result
    nuc = nu * (1.0 + 0.3j) + 0.01j
    M.set_nu(nuc)
    assert M.nu_is_complex
    check(nuc)
    M.set_nu(nu)
    again = [R.apply_batch(V, op=o, M=M) for o, V in (("N", U), ("T", W), ("H", W))]
    assert all(np.array_equal(a, b) for a, b in zip(again, real_bits))


def test_argument_errors_that_need_an_object(lsfc):
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    M, x, h, k, nu = plan8(lsfc)
    R = lsfc.Receivers(x, x, x, k=k, directions=[[0.0, 0.6, 0.8]])
    q, out = np.zeros(512, complex), np.full(1, 7.0 + 0j)
    pq, po = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(word, *args):
        assert lib.lsfc_receivers_apply(*args) == L.LSFC_EINVAL
        assert word in lib.lsfc_last_error().decode(), lib.lsfc_last_error()
        assert out[0] == 7.0

    refused("NULL", R._rc, None, None, po, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    refused("NULL", R._rc, None, pq, None, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    refused("nrhs = 0", R._rc, None, pq, po, 0, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    refused("op 3", R._rc, None, pq, po, 1, 3, L.LSFC_MEM_HOST)
    refused("memspace 2", R._rc, None, pq, po, 1, L.LSFC_OP_N, 2)
    # a plan of another size
    R2 = lsfc.Receivers(x[:7], x, x, k=k, directions=[[0.0, 0.6, 0.8]])
    refused("grid points", R2._rc, M._plan, pq, po, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    # a multi-device plan (two logical ranks on one GPU) and a simulated rank of a slab plan
    from fast_solver_lippmann_schwinger_amd.distributed import MultiDeviceFastM3D
    n = 16
    Mm = MultiDeviceFastM3D(n, 1.0 / n, 3.0, np.zeros(n ** 3), devices=[0, 0])
    try:
        refused("not available on a multi-device plan", R._rc, Mm._plan, pq, po, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    finally:
        Mm.close()
    sim = C.c_void_p()
    nus = np.zeros(n * n * (n // 2))
    L.check(lib.lsfc_dist_sim_plan_create_gv3d(C.byref(sim), n, n, n, 1.0, 3.0, nus.ctypes.data_as(C.c_void_p), 0, 0, 0, 2))
    try:
        refused("not available on a distributed", R._rc, sim, pq, po, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST)
    finally:
        lib.lsfc_plan_destroy(sim)


# ---- the Python wrappers and one solve ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", ["6x5x4", "31x33"])
def test_plane_waves_point_sources_and_linear_operator(lsfc, grid):
    dims, h, origin = GRIDS[grid]
    X = ref.grid_points(dims, origin, h)
    rng = np.random.default_rng(47)
    Rf, th = build(lsfc, grid, FAR, 3)
    a = ref.cvec(rng, 3)
    assert ref.rel(Rf.plane_waves(a), np.exp(1j * K * (X @ th.T)) @ a) <= TOL
    Rp, p = build(lsfc, grid, POINTS, 3)
    D = dense(grid, POINTS, 3)
    assert ref.rel(Rp.point_sources(a), D.T @ a) <= TOL
    e1 = np.array([0, 1, 0], complex)
    assert ref.rel(Rp.point_sources(e1), D[1]) <= TOL                          # one source: the row itself
    A = Rp.aslinearoperator()
    assert A.shape == D.shape
    q = ref.cvec(rng, D.shape[1])
    assert ref.rel(A.matvec(q), D @ q) <= TOL and ref.rel(A.rmatvec(a), D.conj().T @ a) <= TOL
    with pytest.raises(ValueError):
        Rp.plane_waves(a)


def test_scattered_field_of_a_solve(lsfc):
    # examples/example3D.py at 16^3, k = 8: solve for the scattered field on the device, sample it at 12 receivers on a sphere of
    # radius 2 and in the far field, against the reference applied to the same device solution
    import torch
    n, k = 16, 8.0
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    Xg, Yg, Zg = np.meshgrid(x, x, x, indexing="ij")
    X, Y, Z = (A.reshape(-1, order="F") for A in (Xg, Yg, Zg))
    nu = 0.3 * np.exp(-40 * (X ** 2 + Y ** 2 + Z ** 2)) * (np.abs(X) < 0.48) * (np.abs(Y) < 0.48) * (np.abs(Z) < 0.48)
    M = lsfc.buildFastConvolution3D(x, x, x, X, Y, Z, h, k, nu)
    u_inc = torch.from_numpy(np.exp(1j * k * X)).cuda()
    rhs = -(M * u_inc - u_inc)
    u = torch.zeros_like(rhs)
    u, hist = lsfc.gmres_(u, M, rhs, reltol=1e-10, log=True)
    assert hist.isconverged
    u_total = u + u_inc
    th = ref.random_directions(np.random.default_rng(53), 12, 3)
    Rp = lsfc.Receivers(x, x, x, k=k, points=2.0 * th)
    Rf = lsfc.Receivers(x, x, x, k=k, directions=th)
    ut = u_total.cpu().numpy()
    origin = (x[0], x[0], x[0])
    for R, D in ((Rp, ref.dense_points((n, n, n), origin, h, k, 2.0 * th)), (Rf, ref.dense_far((n, n, n), origin, h, k, th))):
        got = R.scattered_field(M, u_total)
        assert got.is_cuda and got.shape == (12,)
        want = -k * k * (D @ (nu * ut))
        err = ref.rel(got.cpu().numpy(), want)
        print(f"  scattered field at 12 receivers: rel l2 {err:.2e}")
        assert err <= TOL
