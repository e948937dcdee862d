"""What the GPU tests of the Krylov solvers share (test_gpu_gmres_kernels.py, test_gpu_gmres_batch.py,
test_gpu_bicgstabl.py, test_gpu_bicgstabl_batch.py): the identity plans, the diag(lambda) preconditioner, and the two
comparisons -- against a long-double reference, and bit for bit between a batch member and its single solve."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import gmres_ref as gr


def _shape(N):
    """(n, m) with n m = N, both <= 8192, as square as possible"""
    best = None
    for n in range(1, 8193):
        if N % n == 0 and N // n <= 8192 and (best is None or abs(n - N // n) < abs(best[0] - best[1])):
            best = (n, N // n)
    assert best is not None, N
    return best


_PLANS = {}


@pytest.fixture(scope="module")
def plan(lsfc):
    """plan(N) -> a cached 2D plan with a ones symbol and nu == 0 whose apply is the identity, bitwise"""
    def get(N):
        if N not in _PLANS:
            n, m = _shape(N)
            M = lsfc.FastM(np.ones((2 * n, 2 * m), complex), np.zeros(N), 2 * n, 2 * m, n, m, 1.0,
                           quadRule="Greengard_Vico", flags=lsfc._lib.LSFC_FLAG_FORCE_ROCFFT)
            x = gr.random_rhs(N, seed=N)
            assert np.array_equal((M * x).view(np.float64), x.view(np.float64)), f"M * x != x at N = {N}"
            _PLANS[N] = M
        return _PLANS[N]
    yield get
    for M in _PLANS.values():
        M.close()
    _PLANS.clear()


def _diag_precond(lsfc, lam):
    """SparsifyingPreconditioner(Msp = I, As = diag(lam)) with identity factors: ldiv!(P, v) = lam .* v on the device"""
    N = lam.size
    eye = sp.identity(N, dtype=complex, format="csr")
    lu = types.SimpleNamespace(perm_r=np.arange(N), perm_c=np.arange(N), L=eye, U=eye)
    return lsfc.SparsifyingPreconditioner(eye, sp.diags(lam, format="csr"), lu=lu)


def _check(label, x, hist, ref, gmap=None, *, history_excess, rtol=1e-10):
    """device result (x on the full vector, ConvergenceHistory) against the reference (x per group); history_excess:
    that of the reference's module"""
    r = np.asarray(hist["resnorm"])
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(x)), f"{label}: non-finite output"
    same = (hist.iters, hist.mvps, hist.isconverged) == (ref["iters"], ref["mvps"], ref["converged"])
    if not same:
        # one iteration apart only where the reference stops within 1e-8 (relative) of the tolerance
        last = ref["resnorm"][-1] if ref["resnorm"].size else ref["beta0"]
        near = abs(last - ref["tol"]) <= 1e-8 * ref["tol"]
        assert near and abs(hist.iters - ref["iters"]) <= 1, \
            f"{label}: iters/mvps/converged {hist.iters}/{hist.mvps}/{hist.isconverged} vs reference " \
            f"{ref['iters']}/{ref['mvps']}/{ref['converged']} ({getattr(hist, 'message', '')})"
    ex, i = history_excess(r, ref, rtol=rtol)
    print(f"{label}: iters {hist.iters}, mvps {hist.mvps}, history excess {ex:.3f}")
    assert ex < 1.0, f"{label}: history entry {i}: {r[i]!r} vs reference {ref['resnorm'][i]!r} ({ex:.2f}x the allowance)"
    xr = ref["x"] if gmap is None else ref["x"][gmap]
    err = float(np.sqrt(np.sum(np.abs(x - xr) ** 2) / np.sum(np.abs(xr) ** 2)))
    assert err < max(1e-10, rtol), f"{label}: x differs from the reference iterate by {err:.2e}"


def _bitwise(tag, X, hs, j, x1, h1):
    assert np.array_equal(X[j].view(np.float64), x1.view(np.float64)), f"{tag}: x of member {j} is not its single solve"
    assert np.array_equal(hs[j]["resnorm"], h1["resnorm"]), f"{tag}: history of member {j}: {hs[j]['resnorm']} vs {h1['resnorm']}"
    assert (hs[j].iters, hs[j].mvps, hs[j].isconverged) == (h1.iters, h1.mvps, h1.isconverged), (tag, j)
