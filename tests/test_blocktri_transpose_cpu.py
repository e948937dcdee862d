"""The transposed block-tridiagonal sweeps and the Python views P.T / P.H, without a GPU.

1. `blocktri_transpose_ref.solve_t_ld` on the blocks of `blocktri_ref.eliminate` against scipy's LU of Msp.T (1e-10, the
   project's bar between independent factorisations), and As.T @ solve_t against the dense (Msp^{-1} As).T.
2. The GMRES step counts that the GPU test's physical cases rest on, from the oracle.
3. The views on a stub object: involution, refusals, the op restored after an exception, and the match rule of `_solve`
   for all nine (operator op, preconditioner op) pairs, with the library's set_op calls and solver entry points recorded
   (the pattern of tests/test_solver_wrappers_cpu.py)."""
import types

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import fast_solver_lippmann_schwinger_amd as pkg
import fast_solver_lippmann_schwinger_amd._lib as L
from fast_solver_lippmann_schwinger_amd.preconditioner import PreconditionerView

import blocktri_cases as bc
import blocktri_transpose_ref as btt
import test_solver_wrappers_cpu as sw
from conftest import rel_err

SMALL = [s for s in bc.SHAPES if s[0] * s[1] <= 3000]
DENSE = [s for s in bc.SHAPES if s[0] * s[1] <= 600]


@pytest.mark.parametrize("shape", SMALL, ids=bc.shape_id)
def test_transposed_sweeps_against_splu(shape):
    b, K, _ = shape
    Msp, _, Sinv = bc.built(shape)
    W = bc.right_hand_sides(b * K, 2, seed=3)
    luT = spla.splu(Msp.T.tocsc())
    X = btt.solve_t_ld(Msp, Sinv, W)
    assert X.shape == W.shape and X.dtype == np.clongdouble
    for j in range(2):
        ref = luT.solve(W[j])
        err = rel_err(X[j].astype(np.complex128), ref), bc.elementwise_err(X[j].astype(np.complex128), ref)
        print(f"{bc.shape_id(shape)}: transposed sweeps vs splu(Msp.T) {err[0]:.2e} in norm, {err[1]:.2e} elementwise")
        assert err[0] <= 1e-10 and err[1] <= 1e-10
    assert np.array_equal(btt.solve_t_ld(Msp, Sinv, W[0]), X[0])             # the (N,) form is the first member


@pytest.mark.parametrize("shape", DENSE, ids=bc.shape_id)
def test_transposed_preconditioner_against_dense(shape):
    b, K, _ = shape
    Msp, As, Sinv = bc.built(shape)
    v = bc.right_hand_sides(b * K, 1, seed=4)[0]
    P = np.linalg.solve(Msp.toarray(), As.toarray())                           # Msp^{-1} As
    got = btt.precond_t(Msp, As, Sinv, v).astype(np.complex128)
    err = rel_err(got, P.T @ v), bc.elementwise_err(got, P.T @ v)
    assert err[0] <= 1e-10 and err[1] <= 1e-10, err
    got_h = btt.precond_h(Msp, As, Sinv, v).astype(np.complex128)
    err = rel_err(got_h, P.conj().T @ v), bc.elementwise_err(got_h, P.conj().T @ v)
    assert err[0] <= 1e-10 and err[1] <= 1e-10, err


@pytest.mark.parametrize("case", sorted(btt.PHYSICAL), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")
def test_oracle_step_counts(case):
    counts, _ = btt.oracle_solves(*case)
    print(case, counts)
    assert counts == btt.PHYSICAL[case]
    for op in ("T", "H"):                                  # what the GPU test asserts of the device: fewer steps with Pl
        assert counts[op][0] < counts[op][1]


# ---- the views ----------------------------------------------------------------------------------------------------------

HANDLE = 0x5eed


class FakeLib(sw.FakeLib):
    """records the two set_op calls as well"""

    def lsfc_plan_set_op(self, plan, op):
        self.events.append(("plan_set_op", op))
        return 0

    def lsfc_precond_set_op(self, pc, op):
        self.events.append(("precond_set_op", sw._addr(pc), op))
        return 0


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib([])
    monkeypatch.setattr(L, "load", lambda: fake)
    return fake


def _parent(lib, fail=False):
    def call(name):
        def f(v):
            lib.events.append((name,))
            if fail:
                raise RuntimeError("planted")
            return v
        return f
    return types.SimpleNamespace(_pc=HANDLE, factor="blocktri", N=sw.N, ldiv_=call("ldiv_"), solve=call("solve"),
                                 ldiv_batch_=call("ldiv_batch_"), solve_batch=call("solve_batch"),
                                 set_stream=lambda s: lib.events.append(("Pl.set_stream", s)))


def _bare():
    """a SparsifyingPreconditioner that holds no handle (as from_operator wraps one)"""
    P = pkg.SparsifyingPreconditioner.__new__(pkg.SparsifyingPreconditioner)
    P._pc, P.factor, P.N = None, "blocktri", sw.N
    return P


def test_views_are_involutions_and_refuse_the_conjugate():
    P = _bare()
    assert isinstance(P.T, PreconditionerView) and P.T._op == L.LSFC_OP_T and P.H._op == L.LSFC_OP_H
    assert P.T.T is P and P.H.H is P and P.transpose().transpose() is P and P.adjoint().adjoint() is P
    assert P.T.parent is P and P.T.N == P.N and P.T._pc is P._pc
    for bad in (lambda: P.H.T, lambda: P.T.H):
        with pytest.raises(NotImplementedError, match="is not offered"):
            bad()


def test_view_of_a_host_lu_object_is_refused():
    P = _bare()
    P.factor = "host"
    for make in (lambda: P.T, lambda: P.H, P.transpose, P.adjoint):
        with pytest.raises(ValueError, match="block-tridiagonal"):
            make()


@pytest.mark.parametrize("op", [L.LSFC_OP_T, L.LSFC_OP_H])
@pytest.mark.parametrize("method", ["ldiv_", "solve", "ldiv_batch_", "solve_batch", "__call__"])
def test_view_sets_the_op_calls_and_restores(lib, op, method):
    view = PreconditionerView(_parent(lib), op)
    v = np.zeros(sw.N, complex)
    out = getattr(view, method)(v)
    inner = "ldiv_" if method == "__call__" else method
    assert lib.events == [("precond_set_op", HANDLE, op), (inner,), ("precond_set_op", HANDLE, L.LSFC_OP_N)]
    assert out is (None if method == "__call__" else v)
    view.set_stream(7)
    assert lib.events[-1] == ("Pl.set_stream", 7)


def test_op_is_restored_after_an_exception(lib):
    view = PreconditionerView(_parent(lib, fail=True), L.LSFC_OP_H)
    with pytest.raises(RuntimeError, match="planted"):
        view.ldiv_(np.zeros(sw.N, complex))
    assert lib.events == [("precond_set_op", HANDLE, L.LSFC_OP_H), ("ldiv_",), ("precond_set_op", HANDLE, L.LSFC_OP_N)]


OPS = [L.LSFC_OP_N, L.LSFC_OP_T, L.LSFC_OP_H]


@pytest.mark.parametrize("solver", ["gmres_", "bicgstabl_", "gmres_batch_", "bicgstabl_batch_"])
@pytest.mark.parametrize("p_op", OPS)
@pytest.mark.parametrize("a_op", OPS)
def test_solve_accepts_a_native_preconditioner_iff_the_ops_match(lib, solver, a_op, p_op):
    A = types.SimpleNamespace(N=sw.N, _plan=None, _op=a_op)
    parent = _parent(lib)
    Pl = parent if p_op == L.LSFC_OP_N else PreconditionerView(parent, p_op)
    x, b = sw._arrays(solver, "numpy")
    if a_op != p_op:
        with pytest.raises(ValueError):
            getattr(pkg, solver)(x, A, b, Pl=Pl)
        assert lib.events == [] and lib.calls == []        # refused before anything reached the library
        return
    getattr(pkg, solver)(x, A, b, Pl=Pl)
    assert len(lib.calls) == 1 and lib.calls[0]["precond_user"] == HANDLE and lib.calls[0]["precond_on_device"] == 1
    assert lib.calls[0]["precond"] == sw._fn_addr(lib._real.lsfc_precond_callback)
    held = [e for e in lib.events if e[0] in ("plan_set_op", "precond_set_op") or e[0].startswith("lsfc_")]
    name = lib.calls[0]["name"]
    if a_op == L.LSFC_OP_N:
        assert held == [(name,)]
    else:                                                  # both ops are held around the call and restored after it
        assert held == [("plan_set_op", a_op), ("precond_set_op", HANDLE, a_op), (name,), ("precond_set_op", HANDLE, L.LSFC_OP_N),
                        ("plan_set_op", L.LSFC_OP_N)]


def test_ops_are_restored_when_the_solver_fails(lib):
    lib.rc, lib.last_error = L.LSFC_EINVAL, sw.EINVAL_PLANTED.encode()
    A = types.SimpleNamespace(N=sw.N, _plan=None, _op=L.LSFC_OP_H)
    x, b = sw._arrays("gmres_", "numpy")
    with pytest.raises(Exception, match=sw.EINVAL_PLANTED):
        pkg.gmres_(x, A, b, Pl=PreconditionerView(_parent(lib), L.LSFC_OP_H))
    assert lib.events[-2:] == [("precond_set_op", HANDLE, L.LSFC_OP_N), ("plan_set_op", L.LSFC_OP_N)]
