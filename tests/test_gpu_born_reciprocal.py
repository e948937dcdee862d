"""GPU tests of the Born operator's reciprocal mode (lsfc_born_contract, csrc/born_contract.hip; lsfc_born_set_mode, csrc/born.hip;
born.py): the two contractions against the numpy.longdouble reference of tests/born_reciprocal_ref.py with bounds that hold for any
order of summation, the operand maps of the matrix instruction with exact integers, the bitwise promises of include/lsfc.h, and
the object in reciprocal mode against tests/born_ref.py at the tolerances of tests/test_gpu_born.py (1e-10 with the solves at
1e-13), against the adjoint-state mode, and for exact adjointness, state and mode changes."""
import ctypes as C
import functools

import numpy as np
import pytest

import born_ref as ref
import born_reciprocal_ref as rr

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = 2.0 ** -52
# a tile is 16 sources x 16 receivers and OP_H takes the receivers in fours: 1, 7, 8, 9, 17, 33 on each side, with the edges 15 / 16
# (a full tile and the last lane of one), 4 / 5 (a full quad of receivers and one more), 32 (two full tiles) and 17 x 49 (eight
# tiles: a launch whose block count is a multiple of eight is dealt out to the dies in another order)
PAIRS = [(1, 1), (7, 9), (8, 8), (9, 7), (17, 1), (1, 17), (33, 8), (8, 33), (17, 49), (16, 16), (15, 17), (17, 15), (32, 4), (5, 32), (33, 33)]
SHAPES = {216: (12, 18), 630: (21, 30), 4096: (64, 64), 4099: (1, 4099)}


def _lib():
    import fast_solver_lippmann_schwinger_amd._lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def plan_of(N):
    """a plan with N grid points (a 2D one with a ones symbol): the contraction takes N, device and stream from it and nothing else"""
    import fast_solver_lippmann_schwinger_amd as lsfc
    n, m = SHAPES[N]
    return lsfc.FastM(np.ones((2 * n, 2 * m), complex), np.zeros(N), 2 * n, 2 * m, n, m, 1.0, quadRule="Greengard_Vico",
                      flags=lsfc._lib.LSFC_FLAG_FORCE_ROCFFT)


def contract(N, U, V, x, op, scale=1.0, device=False, **kw):
    import fast_solver_lippmann_schwinger_amd as lsfc
    if not device:
        return lsfc.born_contract(plan_of(N), U, V, x, op=op, scale=scale, **kw)
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()             # noqa: E731
    if kw.get("accumulate") is not None:
        kw["accumulate"] = t(kw["accumulate"])
    xin = np.asarray(x) if op == "N" else np.asarray(x, dtype=complex).reshape(-1)
    out = lsfc.born_contract(plan_of(N), t(U), t(V), t(xin), op=op, scale=scale, **kw)
    plan_of(N).synchronize()
    return out.cpu().numpy()


# ---- lsfc_born_contract --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", list(SHAPES))
def test_contract_against_longdouble(N):
    L, _ = _lib()
    rng = np.random.default_rng(N)
    scale = complex(-2.25, 0.75)
    pairs = PAIRS if N in (630, 4099) else PAIRS[:9]
    worst_n = worst_h = 0.0
    for n, (nsrc, nrecv) in enumerate(pairs):
        device = bool(n % 2)
        U, V = ref.cvec(rng, nsrc, N), ref.cvec(rng, nrecv, N)
        for x in (rng.standard_normal(N), ref.cvec(rng, N)):
            got = contract(N, U, V, x, "N", scale, device)
            re, im, mag = rr.contract_n_ld(U, V, x, scale)
            share = float((rr.err_ld(got, re, im) / ((N + 16) * EPS * mag)).max())
            worst_n = max(worst_n, share)
            assert got.shape == (nsrc, nrecv) and share <= 1.0, (nsrc, nrecv, share)
        r = ref.cvec(rng, nsrc, nrecv)
        got = contract(N, U, V, r, "H", scale, device)
        re, im, mag = rr.contract_h_ld(U, V, r, scale)
        share = float((rr.err_ld(got, re, im) / ((nsrc * nrecv + 16) * EPS * mag)).max())
        worst_h = max(worst_h, share)
        assert got.dtype == np.complex128 and share <= 1.0, (nsrc, nrecv, share)
        # REAL is the real part bit for bit; ACCUMULATE adds onto what out held (its rounding: one more addition of |start|)
        real = contract(N, U, V, r, "H", scale, device, real=True)
        assert real.dtype == np.float64 and np.array_equal(real, got.real)
        start = ref.cvec(rng, N)
        acc = contract(N, U, V, r, "H", scale, device, accumulate=start)
        re, im, _ = rr.contract_h_ld(U, V, r, scale, start)
        assert float((rr.err_ld(acc, re, im) / ((nsrc * nrecv + 16) * EPS * (mag + np.abs(start)))).max()) <= 1.0
        acc_real = contract(N, U, V, r, "H", scale, device, real=True, accumulate=start.real.copy())
        assert np.array_equal(acc_real, acc.real)
    print(f"  N {N}: largest share of the bound, OP_N {worst_n:.4f}, OP_H {worst_h:.4f}")


@pytest.mark.parametrize("nsrc,nrecv", [(8, 8), (17, 9), (16, 33), (49, 17)])
def test_operand_maps_with_exact_integers(nsrc, nrecv):
    # small integers without a symmetry between the members, the parts or the points: every product and every partial sum is an
    # integer below 2^53, so the result is the integer result exactly, whatever the order; a transposed or misplaced operand is not
    N = 630
    rng = np.random.default_rng(nsrc * 100 + nrecv)
    ints = lambda *shape: rng.integers(-7, 8, shape).astype(float) + 1j * rng.integers(-7, 8, shape).astype(float)    # noqa: E731
    U, V = ints(nsrc, N), ints(nrecv, N)
    U[:, 0] += 16 * np.arange(nsrc)
    V[:, 1] += 32j * np.arange(nrecv)
    scale = complex(2.0, -3.0)
    for x in (rng.integers(-5, 6, N).astype(float), ints(N)):
        want = scale * np.einsum("i,si,ri->sr", x, U, V)
        got = contract(N, U, V, x, "N", scale)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    r = ints(nsrc, nrecv)
    want = np.conj(scale) * np.einsum("si,ri,sr->i", np.conj(U), np.conj(V), r)
    got = contract(N, U, V, r, "H", scale)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(contract(N, U, V, r, "H", scale, device=True), want)


@pytest.mark.parametrize("N", [630, 4099])
def test_contract_bits(N):
    rng = np.random.default_rng(11)
    nsrc, nrecv = 33, 17
    U, V, x = ref.cvec(rng, nsrc, N), ref.cvec(rng, nrecv, N), ref.cvec(rng, N)
    scale = complex(-9.0, 0.5)
    full = contract(N, U, V, x, "N", scale)
    assert np.array_equal(full, contract(N, U, V, x, "N", scale)), "two calls"
    assert np.array_equal(full, contract(N, U, V, x, "N", scale, device=True)), "host and device vectors"
    # out[s, r] alone: other members, the counts and the pair's place do not enter its bits
    for s, r in ((0, 0), (7, 16), (15, 3), (16, 15), (32, 16), (20, 9)):
        assert np.array_equal(contract(N, U[s:s + 1], V[r:r + 1], x, "N", scale)[0, 0], full[s, r]), (s, r)
    V49 = ref.cvec(rng, 49, N)                              # 2 x 4 tiles: the launch that is dealt out to the dies in another order
    wide = contract(N, U[:17], V49, x, "N", scale)
    for s, r in ((16, 48), (3, 20), (0, 0)):
        assert np.array_equal(contract(N, U[s:s + 1], V49[r:r + 1], x, "N", scale)[0, 0], wide[s, r]), (s, r)
    ps, pr = rng.permutation(nsrc), rng.permutation(nrecv)
    assert np.array_equal(contract(N, U[ps], V[pr], x, "N", scale), full[np.ix_(ps, pr)]), "members permuted"
    xr = rng.standard_normal(N)
    assert np.array_equal(contract(N, U[ps], V, xr, "N", scale), contract(N, U, V, xr, "N", scale)[ps]), "real input, members permuted"
    # OP_H: the promise of include/lsfc.h -- a cut at a multiple of 16 sources through ACCUMULATE gives the bits of one call
    r = ref.cvec(rng, nsrc, nrecv)
    one = contract(N, U, V, r, "H", scale)
    assert np.array_equal(one, contract(N, U, V, r, "H", scale)), "two calls"
    assert np.array_equal(one, contract(N, U, V, r, "H", scale, device=True)), "host and device vectors"
    for cut in (16, 32):
        g = contract(N, U[:cut], V, r[:cut], "H", scale)
        g = contract(N, U[cut:], V, r[cut:], "H", scale, accumulate=g)
        assert np.array_equal(one, g), cut
    g = contract(N, U[:16], V, r[:16], "H", scale, real=True)
    g = contract(N, U[16:], V, r[16:], "H", scale, real=True, accumulate=g)
    assert np.array_equal(g, one.real) and np.array_equal(contract(N, U, V, r, "H", scale, real=True), one.real)


# ---- the object ------------------------------------------------------------------------------------------------------------------

def tb():
    import test_gpu_born
    return test_gpu_born


def check_object(lsfc, name, kind, nsrc, nrecv, complex_nu, device=False, **kw):
    case, G = tb().green(lsfc, name)
    nu = ref.nu_of(case, complex_nu)
    M = tb().operator_of(lsfc, case, nu)
    R, Rd = tb().receivers_of(lsfc, case, kind, nrecv)
    U_inc = ref.plane_waves(case, nsrc)
    k = case.k
    B = lsfc.BornOperator(M, R, U_inc, reltol=1e-13, mode="reciprocal", **kw)
    assert B.converged and B.mode == "reciprocal", B.message
    assert len(B.receiver_history) == nrecv and all(h.isconverged for h in B.receiver_history)
    chunk = B.info()["chunk"]
    info = B.receiver_info()
    assert (info["nrecv"], info["solves"], info["first_not_converged"]) == (nrecv, -(-nrecv // chunk), -1)
    assert info["mvps"] == sum(h.mvps for h in B.receiver_history) and info["receiver_field_bytes"] == nrecv * B.N * 16
    U, d = ref.forward(G, Rd, nu, k, U_inc)
    figures = {"data": ref.rel(B.data, d), "V": ref.rel(B.receiver_fields.cpu().numpy(), rr.receiver_fields(G, Rd, nu, k))}
    if device:
        import torch
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()         # noqa: E731
        back = lambda t: t.cpu().numpy()                                         # noqa: E731
    else:
        to = back = lambda a: a                                                  # noqa: E731
    results = {}
    for cd in (False, True):
        dnu = ref.perturbation(case, complex_=cd)
        got = back(B * to(dnu))
        assert got.shape == (nsrc, nrecv) and B.converged
        assert (B.info()["solves"], B.info()["mvps"]) == (0, 0) and all(h.isconverged and h.iters == 0 for h in B.history)
        figures[f"J complex dnu {cd}"] = ref.rel(got, ref.J(G, Rd, nu, k, U, dnu))
        assert np.array_equal(got, back(B.apply(to(dnu)))), "two calls, the same bits"
        results[f"J{cd}"] = got
    r = ref.cvec(np.random.default_rng(21), nsrc, nrecv)
    g = back(B.H * to(r))
    assert (B.info()["solves"], B.info()["mvps"]) == (0, 0)
    figures["JH"] = ref.rel(g, ref.JH(G, Rd, nu, k, U, r))
    assert np.array_equal(back(B.adjoint(to(r), real=True)), g.real)
    d_obs = ref.forward(G, Rd, 1.2 * nu, k, U_inc)[1]
    phi, grad = B.misfit(d_obs)
    phi_ref, grad_ref = ref.misfit(G, Rd, nu, k, U_inc, d_obs)
    assert grad.dtype == (np.complex128 if complex_nu else np.float64)
    figures["phi"], figures["grad"] = abs(phi - phi_ref) / phi_ref, ref.rel(grad, grad_ref)
    # the two modes of the library
    B.set_mode("adjoint-state")
    assert B.mode == "adjoint-state" and B.receiver_info()["receiver_field_bytes"] == 0
    figures["modes J"] = ref.rel(B * ref.perturbation(case, complex_=True), results["JTrue"])
    assert B.info()["solves"] > 0
    figures["modes JH"] = ref.rel(B.H * r, g)
    print("  " + ", ".join(f"{n} {v:.1e}" for n, v in figures.items()))
    for fname, v in figures.items():
        assert v <= TOL, (fname, v)
    B.close(), R.close(), M.close()
    return chunk


@pytest.mark.parametrize("complex_nu", [False, True])
@pytest.mark.parametrize("kind", [ref.FAR, ref.POINTS])
@pytest.mark.parametrize("name", ["6^3", "8^3-kh0.8", "10x9x7", "10^2"])
def test_parity_on_every_grid(lsfc, name, kind, complex_nu):
    check_object(lsfc, name, kind, 3, 7, complex_nu, device=(kind == ref.POINTS))


@pytest.mark.parametrize("solver", ["gmres", "bicgstabl"])
@pytest.mark.parametrize("nsrc,nrecv,chunk", [(1, 1, None), (1, 9, 1), (3, 17, 2), (9, 7, 2), (9, 17, None), (3, 9, 1)])
def test_parity_for_every_count_chunking_and_solver(lsfc, nsrc, nrecv, chunk, solver):
    used = check_object(lsfc, "6^3", ref.FAR, nsrc, nrecv, nsrc == 3, device=(nsrc == 9), chunk=chunk, solver=solver, l=2)
    assert used == (min(chunk, nsrc) if chunk else nsrc)


def test_exact_adjointness_at_a_loose_tolerance(lsfc):
    case = ref.CASES["8^3-kh0.8"]
    M = tb().operator_of(lsfc, case, ref.nu_of(case, True))
    R, _ = tb().receivers_of(lsfc, case, ref.FAR, 9)
    B = lsfc.BornOperator(M, R, ref.plane_waves(case, 3), reltol=1e-3, mode="reciprocal")
    assert B.converged
    dnu = ref.perturbation(case, complex_=True)
    r = ref.cvec(np.random.default_rng(4), 3, 9)

    def defect():
        Jd, g = B * dnu, B.H * r
        return abs(np.vdot(r, Jd) - np.vdot(g, dnu)) / (np.linalg.norm(r) * np.linalg.norm(Jd))

    recip = defect()
    B.set_mode("adjoint-state")
    adj = defect()
    print(f"  dot-identity defect at reltol 1e-3: reciprocal {recip:.2e}, adjoint-state {adj:.2e}")
    assert recip <= 1e-12, recip
    assert adj > 1e-8, adj                                  # what the mode buys: the old one is adjoint to the solver tolerance only
    B.close(), R.close(), M.close()


def test_no_solves_no_state_and_mode_changes(lsfc):
    import sparsify_cases as sc
    L, lib = _lib()
    case = ref.Case((4, 4, 4), 4.0, 0.3)
    assert sc.find("gv3", case.dims)
    ref.CASES["4^3"] = case
    G = ref.dense_G("4^3")
    nu = ref.nu_of(case)
    M = tb().operator_of(lsfc, case, nu)
    P = lsfc.SparsifyingPreconditioner.from_operator(M)
    R, Rd = tb().receivers_of(lsfc, case, ref.FAR, 5)
    U_inc = ref.plane_waves(case, 3)
    k = case.k
    dnu, r = ref.perturbation(case), ref.cvec(np.random.default_rng(3), 3, 5)
    B = lsfc.BornOperator(M, R, U_inc, Pl=P, reltol=1e-13)
    assert B.mode == "adjoint-state" and B.receiver_history == []
    with pytest.raises(L.LsfcError, match="outside reciprocal mode"):
        B.receiver_fields
    old_j, old_h = B * dnu, B.H * r
    # a switch with a background present: working applies without a new set_background
    B.set_mode("reciprocal")
    assert B.converged and B.receiver_info()["solves"] == 2 and B.receiver_info()["receiver_field_bytes"] == 5 * 64 * 16
    U, _ = ref.forward(G, Rd, nu, k, U_inc)
    sweeps = P.batch_info()["sweeps"]
    # the plan's and the preconditioner's op are what they were, under N and under H, and nothing is applied
    for op in (L.LSFC_OP_N, L.LSFC_OP_H):
        L.check(lib.lsfc_plan_set_op(M._plan, op))
        L.check(lib.lsfc_precond_set_op(P._pc, op))
        try:
            assert ref.rel(B * dnu, ref.J(G, Rd, nu, k, U, dnu)) <= TOL and tb().ops_of(M, P) == (op, op)
            assert ref.rel(B.H * r, ref.JH(G, Rd, nu, k, U, r)) <= TOL and tb().ops_of(M, P) == (op, op)
            assert (B.info()["solves"], B.info()["mvps"]) == (0, 0) and P.batch_info()["sweeps"] == sweeps
        finally:
            L.check(lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N))
            L.check(lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_N))
    assert B.receiver_info()["solves"] == 2                 # still those of the set-up: 5 receivers, 3 at a time
    # back: V is released and the old results return bit for bit
    B.set_mode("adjoint-state")
    assert B.receiver_info()["receiver_field_bytes"] == 0
    assert np.array_equal(B * dnu, old_j) and np.array_equal(B.H * r, old_h)
    # update refreshes V
    B.set_mode("reciprocal")
    nu2 = 1.3 * nu
    B.update(nu2)
    U2, d2 = ref.forward(G, Rd, nu2, k, U_inc)
    assert B.converged and ref.rel(B.data, d2) <= TOL
    assert ref.rel(B * dnu, ref.J(G, Rd, nu2, k, U2, dnu)) <= TOL and ref.rel(B.H * r, ref.JH(G, Rd, nu2, k, U2, r)) <= TOL
    B.update(nu)
    B.close()
    # receiver solves capped at maxiter = 1 (reltol = 0, restart = 1: see tests/test_gpu_born.py): LSFC_ENOTCONV names a receiver and the
    # stage beside the source, B.converged is False, V is kept and the outputs are written
    B1 = lsfc.BornOperator(M, R, U_inc, Pl=P, reltol=0.0, restart=1, maxiter=1, mode="reciprocal")
    assert not B1.converged and "source 0" in B1.message and "receiver 0" in B1.message and "receiver-field solve on M" in B1.message
    assert len(B1.receiver_history) == 5 and not any(h.isconverged for h in B1.receiver_history)
    assert B1.receiver_info()["first_not_converged"] == 0 and tb().ops_of(M, P) == (L.LSFC_OP_N, L.LSFC_OP_N)
    assert np.abs(B1.receiver_fields.cpu().numpy()).min(axis=1).max() > 0 and np.all(np.isfinite(B1.data))
    out = B1 * dnu
    assert np.all(np.isfinite(out)) and np.abs(out).max() > 0
    # the switch itself: its message is about the receivers alone
    B1.set_mode("adjoint-state")
    B1.set_mode("reciprocal")
    assert not B1.converged and B1.message.startswith("lsfc_born_set_mode: receiver 0") and "receiver-field solve on M" in B1.message
    assert np.all(np.isfinite(B1.H * r))
    B1.close()
    # a host-LU object has no transposed apply: J runs in reciprocal mode and is still refused in adjoint-state mode
    Plu = lsfc.SparsifyingPreconditioner(*lsfc.sparsifying_pair(M))
    B2 = lsfc.BornOperator(M, R, U_inc, Pl=Plu, reltol=1e-13, mode="reciprocal")
    assert B2.converged and ref.rel(B2 * dnu, ref.J(G, Rd, nu, k, U, dnu)) <= TOL
    assert ref.rel(B2.H * r, ref.JH(G, Rd, nu, k, U, r)) <= TOL
    B2.set_mode("adjoint-state")
    with pytest.raises(L.LsfcError) as e:
        B2 * dnu
    assert e.value.code == L.LSFC_EINVAL and "cannot follow" in str(e.value)
    B2.close()
    P.close(), R.close(), M.close()
