"""What gmres_, gmres_batch_, bicgstabl_ and bicgstabl_batch_ hand to the library, and what they make of its answer,
without a GPU: the library's four solver entry points and lsfc_plan_set_stream are replaced by recorders that copy out
the option struct and the scalar arguments, call a caller's preconditioner on a small host vector, and plant resnorm,
results and status.  Everything else (lsfc_precond_callback, lsfc_last_error) is the real library."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import fast_solver_lippmann_schwinger_amd as pkg
import fast_solver_lippmann_schwinger_amd._lib as L
import fast_solver_lippmann_schwinger_amd.operators as ops

N = 6
GMRES_FIELDS = ["restart", "maxiter", "reltol", "abstol", "orth", "initially_zero", "precond_user", "precond_on_device"]
BICG_FIELDS = ["l", "max_mv_products", "reltol", "abstol", "initially_zero", "precond_user", "precond_on_device", "r_shadow"]
EINVAL_PLANTED = "planted error text"


def _addr(arg):
    """the address a ctypes argument stands for: byref(obj), a ctypes instance, a c_void_p or an int"""
    if arg is None:
        return None
    if hasattr(arg, "_obj"):
        return C.addressof(arg._obj)
    if isinstance(arg, C.c_void_p):
        return arg.value
    if isinstance(arg, int):
        return arg
    return C.addressof(arg)


def _fn_addr(fn):
    return C.cast(fn, C.c_void_p).value if fn else None


class FakeLib:
    """delegates to the real library except for the four solver calls and lsfc_plan_set_stream"""

    def __init__(self, events):
        self._real = L.load()
        self.events = events
        self.calls = []
        self.rc = 0
        self.iters = [3, 2, 50]            # planted per row (50: beyond every cap used with log=True below but one)
        self.codes = [(L.LSFC_BICG_CONVERGED, 3)] * 3
        self.last_error = None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def lsfc_last_error(self):
        return self.last_error if self.last_error is not None else self._real.lsfc_last_error()

    def lsfc_plan_set_stream(self, plan, stream):
        self.events.append(("plan_set_stream", _addr(plan), _addr(stream)))
        return 0

    def _solve(self, name, fields, plan, px, pb, nrhs, opts, resnorm, cap, res, status, memspace):
        o = C.cast(_addr(opts), C.POINTER(L.BicgstablOpts if "bicg" in name else L.GmresOpts)).contents
        rec = {f: getattr(o, f) for f in fields}
        rec.update(name=name, plan=_addr(plan), px=_addr(px), pb=_addr(pb), nrhs=nrhs, cap=cap, memspace=memspace,
                   precond=_fn_addr(o.precond), cb_rc=None, cb_vec=None)
        # read b and r_shadow through the pointers while the call is on: a copy that was let go would not hold its values
        count = N * (1 if nrhs is None else max(int(nrhs), 1))
        rec["b"] = np.ctypeslib.as_array((C.c_double * (2 * count)).from_address(rec["pb"])).view(np.complex128).copy()
        if "bicg" in name and o.r_shadow:
            rec["shadow"] = np.ctypeslib.as_array((C.c_double * (2 * count)).from_address(o.r_shadow)).view(np.complex128).copy()
        if "bicg" in name:
            rec["reserved"] = list(o.reserved)
        self.events.append((name,))
        self.calls.append(rec)
        rc = self.rc
        if rec["precond"] is not None and rec["precond"] != _fn_addr(self._real.lsfc_precond_callback):
            v = (np.arange(N) + 1.0).astype(np.complex128)
            rec["cb_rc"] = o.precond(o.precond_user, v.ctypes.data_as(C.POINTER(C.c_double)), N)
            rec["cb_vec"] = v
            if rec["cb_rc"] != 0:
                rc = L.LSFC_EINVAL
        rows = 1 if nrhs is None else max(int(nrhs), 1)
        rn = np.ctypeslib.as_array((C.c_double * (rows * cap)).from_address(_addr(resnorm))).reshape(rows, cap)
        rs = (L.GmresResult * rows).from_address(_addr(res))
        for j in range(rows):
            rn[j, :] = 100.0 * (j + 1) + np.arange(cap)
            rs[j].iters, rs[j].mvps, rs[j].converged, rs[j].final_resnorm = self.iters[j], 7 + j, (j + 1) % 2, 0.5
        if status is not None:
            st = np.ctypeslib.as_array((C.c_int64 * (2 * rows)).from_address(_addr(status))).reshape(rows, 2)
            for j in range(rows):
                st[j] = self.codes[j]
        return rc

    def lsfc_gmres(self, plan, px, pb, opts, resnorm, cap, res, memspace):
        return self._solve("lsfc_gmres", GMRES_FIELDS, plan, px, pb, None, opts, resnorm, cap, res, None, memspace)

    def lsfc_gmres_batch(self, plan, px, pb, nrhs, opts, resnorm, cap, res, memspace):
        return self._solve("lsfc_gmres_batch", GMRES_FIELDS, plan, px, pb, nrhs, opts, resnorm, cap, res, None, memspace)

    def lsfc_bicgstabl(self, plan, px, pb, opts, resnorm, cap, res, memspace):
        return self._solve("lsfc_bicgstabl", BICG_FIELDS, plan, px, pb, None, opts, resnorm, cap, res, None, memspace)

    def lsfc_bicgstabl_batch(self, plan, px, pb, nrhs, opts, resnorm, cap, res, status, memspace):
        return self._solve("lsfc_bicgstabl_batch", BICG_FIELDS, plan, px, pb, nrhs, opts, resnorm, cap, res, status, memspace)


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib([])
    monkeypatch.setattr(L, "load", lambda: fake)
    return fake


A = types.SimpleNamespace(N=N, _plan=None)

# (wrapper, flavour of the arrays)
SINGLE = [("gmres_", "numpy"), ("gmres_", "torch"), ("bicgstabl_", "numpy"), ("bicgstabl_", "torch")]
BATCH = [("gmres_batch_", "numpy"), ("gmres_batch_", "torch"), ("bicgstabl_batch_", "numpy"), ("bicgstabl_batch_", "torch")]
ALL = SINGLE + BATCH


def _is_batch(name):
    return name.endswith("batch_")


def _arrays(name, kind, nrhs=2):
    shape = (nrhs, N) if _is_batch(name) else (N,)
    x, b = np.zeros(shape, np.complex128), np.ones(shape, np.complex128)
    return (torch.from_numpy(x), torch.from_numpy(b)) if kind == "torch" else (x, b)


def _ptr(a):
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _run(name, kind, nrhs=2, **kw):
    x, b = _arrays(name, kind, nrhs)
    return x, b, getattr(pkg, name)(x, A, b, **kw)


class FakeCudaTensor:
    """what the wrappers read of a torch CUDA tensor (no GPU here): only ever refused, never handed to the library"""
    __module__ = "torch"
    dtype, is_cuda, device = torch.complex128, True, "cuda:0"

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 4096

    def reshape(self, *_):
        return FakeCudaTensor(self.numel())


# ---------------------------------------------------------------------------- options, caps, pointers
@pytest.mark.parametrize("name,kind", ALL)
def test_defaults_reach_the_struct(lib, name, kind):
    x, b, out = _run(name, kind)
    assert out is x                                                     # log=False: the caller's own object
    (c,) = lib.calls
    assert c["name"] == "lsfc_" + name.rstrip("_") and c["plan"] is None and c["memspace"] == L.LSFC_MEM_HOST
    assert c["nrhs"] == (2 if _is_batch(name) else None)
    assert c["px"] == _ptr(x) and c["pb"] == _ptr(b)                    # no copies of contiguous complex128 input
    assert c["reltol"] == -1.0 and c["abstol"] == 0.0 and c["initially_zero"] == 0
    assert c["precond"] is None and c["precond_user"] is None and c["precond_on_device"] == 0
    if "gmres" in name:
        assert (c["restart"], c["maxiter"], c["orth"]) == (0, 0, L.LSFC_ORTH_MGS)
        assert c["cap"] == N
    else:
        assert (c["l"], c["max_mv_products"], c["r_shadow"], c["reserved"]) == (2, 0, None, [0, 0, 0, 0])
        assert c["cap"] == N // 4 + 2
    assert lib.events == [(c["name"],)]                                 # no stream moves without a device object


@pytest.mark.parametrize("name,kind", [p for p in ALL if "gmres" in p[0]])
def test_gmres_options(lib, name, kind):
    for orth, code in [("ModifiedGramSchmidt", L.LSFC_ORTH_MGS), ("ClassicalGramSchmidt", L.LSFC_ORTH_CGS), ("DGKS", L.LSFC_ORTH_DGKS)]:
        _run(name, kind, abstol=1e-3, reltol=1e-5, restart=4, maxiter=9, initially_zero=True, orth_meth=orth)
        c = lib.calls[-1]
        assert (c["restart"], c["maxiter"], c["reltol"], c["abstol"], c["orth"], c["initially_zero"]) == (4, 9, 1e-5, 1e-3, code, 1)
        assert c["cap"] == 9
    with pytest.raises(KeyError):
        _run(name, kind, orth_meth="Householder")
    _run(name, kind, nrhs=1, maxiter=(1 << 20) + 5)
    assert lib.calls[-1]["cap"] == 1 << 20 and lib.calls[-1]["maxiter"] == (1 << 20) + 5


@pytest.mark.parametrize("name,kind", [p for p in ALL if "bicg" in p[0]])
def test_bicgstabl_options(lib, name, kind):
    _run(name, kind, l=3, max_mv_products=40, abstol=1e-3, reltol=1e-5, initially_zero=True)
    c = lib.calls[-1]
    assert (c["l"], c["max_mv_products"], c["reltol"], c["abstol"], c["initially_zero"]) == (3, 40, 1e-5, 1e-3, 1)
    assert c["cap"] == 40 // 6 + 2 and c["reserved"] == [0, 0, 0, 0]
    _run(name, kind, l=0)                                               # the library refuses l = 0; the cap must not divide by it
    assert lib.calls[-1]["l"] == 0 and lib.calls[-1]["cap"] == N // 2 + 2
    _run(name, kind, l=1, max_mv_products=0)                            # 0: the library's default, N
    assert lib.calls[-1]["cap"] == N // 2 + 2
    _run(name, kind, nrhs=1, l=1, max_mv_products=1 << 22)
    assert lib.calls[-1]["cap"] == 1 << 20
    # r_shadow: the caller's memory, in the memory space of x
    x, b = _arrays(name, kind)
    sh = np.full(x.shape, 2.0 + 0j)
    sh = torch.from_numpy(sh) if kind == "torch" else sh
    getattr(pkg, name)(x, A, b, r_shadow=sh)
    assert lib.calls[-1]["r_shadow"] == _ptr(sh) and np.all(lib.calls[-1]["shadow"] == 2.0)
    if kind == "numpy":                                                 # a converted copy: alive, with its values, during the call
        getattr(pkg, name)(x, A, b, r_shadow=[[3.0] * N] * 2 if _is_batch(name) else [3.0] * N)
        assert lib.calls[-1]["r_shadow"] is not None and np.all(lib.calls[-1]["shadow"] == 3.0)
    ncalls = len(lib.calls)
    if kind == "torch" or not _is_batch(name):                          # (rows of a numpy batch are numpy: always host memory)
        with pytest.raises(TypeError, match="r_shadow and .* same memory space"):
            getattr(pkg, name)(x, A, b, r_shadow=FakeCudaTensor(*x.shape))
    with pytest.raises((ValueError, TypeError)):
        getattr(pkg, name)(x, A, b, r_shadow=sh.reshape(-1)[:N - 1])
    assert len(lib.calls) == ncalls


# ---------------------------------------------------------------------------- the three preconditioner routes
@pytest.mark.parametrize("name,kind", ALL)
def test_host_callable(lib, name, kind):
    seen = []

    def Pl(v):
        seen.append((type(v), v.dtype, v.shape))
        v *= 2.0

    _run(name, kind, Pl=Pl)
    c = lib.calls[-1]
    assert c["precond"] is not None and c["precond_user"] is None and c["precond_on_device"] == 0
    assert c["cb_rc"] == 0 and seen == [(np.ndarray, np.dtype(np.complex128), (N,))]
    assert np.array_equal(c["cb_vec"], 2.0 * (np.arange(N) + 1.0))      # in place, on the library's own vector
    assert lib.events == [(c["name"],)]


@pytest.mark.parametrize("name,kind", [p for p in ALL if p[0] != "gmres_batch_"])
def test_device_callable(lib, monkeypatch, name, kind):
    views = []

    def view(ptr, n):
        views.append((ptr, n))
        return np.ctypeslib.as_array((C.c_double * (2 * n)).from_address(ptr)).view(np.complex128)

    monkeypatch.setattr(ops, "_device_view", view)                      # (torch cannot alias a pointer without a GPU)
    _run(name, kind, Pl=lambda v: np.multiply(v, 3.0, out=v), Pl_on_device=True)
    c = lib.calls[-1]
    assert c["precond"] is not None and c["precond_user"] is None and c["precond_on_device"] == 1
    assert c["cb_rc"] == 0 and views == [(c["cb_vec"].ctypes.data, N)]
    assert np.array_equal(c["cb_vec"], 3.0 * (np.arange(N) + 1.0))


def test_gmres_batch_has_no_device_callable():
    import inspect
    assert "Pl_on_device" not in inspect.signature(pkg.gmres_batch_).parameters
    for name in ("gmres_", "bicgstabl_", "bicgstabl_batch_"):
        assert inspect.signature(getattr(pkg, name)).parameters["Pl_on_device"].default is False


@pytest.mark.parametrize("name,kind", ALL)
def test_library_object(lib, name, kind):
    handle = C.c_void_p(0x5150)
    Pl = types.SimpleNamespace(_pc=handle, set_stream=lambda s: lib.events.append(("Pl.set_stream", s)))
    kw = {} if name == "gmres_batch_" else {"Pl_on_device": False}
    _run(name, kind, Pl=Pl, **kw)
    c = lib.calls[-1]
    assert c["precond"] == _fn_addr(L.load()._real.lsfc_precond_callback)
    assert c["precond_user"] == 0x5150 and c["precond_on_device"] == 1 and c["cb_rc"] is None
    # host vectors: plan and preconditioner both go to the null stream, in this order, before the solve
    assert lib.events == [("plan_set_stream", None, None), ("Pl.set_stream", 0), (c["name"],)]


@pytest.mark.parametrize("name,kind", ALL)
def test_raising_callable(lib, name, kind):
    class Boom(Exception):
        pass

    def Pl(v):
        raise Boom("from the preconditioner")

    with pytest.raises(Boom):                                           # not the LsfcError of the code the call returned
        _run(name, kind, Pl=Pl, log=True)
    assert lib.calls[-1]["cb_rc"] == 1


# ---------------------------------------------------------------------------- return codes and histories
@pytest.mark.parametrize("name,kind", ALL)
def test_return_codes(lib, name, kind):
    lib.last_error = EINVAL_PLANTED.encode()
    for rc in (L.LSFC_EINVAL, L.LSFC_ENOMEM, L.LSFC_ENODEV, 3):
        lib.rc = rc
        with pytest.raises(L.LsfcError, match=EINVAL_PLANTED) as e:
            _run(name, kind)
        assert e.value.code == rc
    lib.rc = L.LSFC_ENOTCONV
    if _is_batch(name):
        with pytest.raises(L.LsfcError):
            _run(name, kind)
    else:
        x, b, out = _run(name, kind)
        assert out is x
        x, b, (out, hist) = _run(name, kind, log=True)
        assert out is x and hist.iters == 3
        if name == "bicgstabl_":
            assert hist.message == EINVAL_PLANTED
    assert len(lib.calls) == (5 if _is_batch(name) else 6)              # every refusal came after the call


def _check_history(h, row, cap, iters):
    kept = min(iters, cap)
    r = h["resnorm"]
    assert h[":resnorm"] is r and r.flags.owndata and r.dtype == np.float64
    assert np.array_equal(r, 100.0 * (row + 1) + np.arange(kept))
    assert (h.iters, h.mvps, h.isconverged) == (iters, 7 + row, row % 2 == 0)
    assert type(h.iters) is int and type(h.mvps) is int and type(h.isconverged) is bool


@pytest.mark.parametrize("name,kind", SINGLE)
def test_history_of_a_single_solve(lib, name, kind):
    for iters in (3, 50, 0):
        lib.iters = [iters]
        x, b, (out, h) = _run(name, kind, log=True)
        assert out is x and isinstance(h, pkg.ConvergenceHistory)
        _check_history(h, 0, lib.calls[-1]["cap"], iters)
        if name == "bicgstabl_":
            assert h.message == ""


@pytest.mark.parametrize("name,kind", BATCH)
def test_histories_of_a_batch(lib, name, kind):
    for nrhs in (1, 3):
        x, b, (out, hs) = _run(name, kind, nrhs=nrhs, log=True)
        assert out is x and len(hs) == nrhs and lib.calls[-1]["nrhs"] == nrhs
        for j, h in enumerate(hs):
            _check_history(h, j, lib.calls[-1]["cap"], lib.iters[j])


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_bicgstabl_batch_status_and_message(lib, kind):
    reasons = {L.LSFC_BICG_RHO: "rho is not finite", L.LSFC_BICG_SIGMA: "sigma is zero or not finite",
               L.LSFC_BICG_BETA: "beta = rho / sigma is not finite", L.LSFC_BICG_ALPHA: "alpha = rho / sigma is not finite",
               L.LSFC_BICG_GAMMA: "gamma (singular or non-finite Gram matrix)", L.LSFC_BICG_RESIDUAL: "the residual norm is not finite"}
    want = {L.LSFC_BICG_CONVERGED: "", L.LSFC_BICG_MAX_MV: "bicgstabl: max_mv_products reached without convergence"}
    for code, text in reasons.items():
        want[code] = f"bicgstabl: breakdown in cycle 5: {text}; x is the last finite iterate"
    want[9] = "bicgstabl: breakdown in cycle 5: 9; x is the last finite iterate"       # a code this binding does not know
    codes = sorted(want)
    for i in range(0, len(codes), 3):
        part = codes[i:i + 3]
        lib.codes = [(c, 5) for c in part]
        _, _, (_, hs) = _run("bicgstabl_batch_", kind, nrhs=len(part), log=True)
        for c, h in zip(part, hs):
            assert h.status == (c, 5) and h.message == want[c]
            assert type(h.status[0]) is int and type(h.status[1]) is int


# ---------------------------------------------------------------------------- what the wrappers refuse themselves
@pytest.mark.parametrize("name,kind", SINGLE)
def test_single_refusals(lib, name, kind):
    f = getattr(pkg, name)
    x, b = _arrays(name, kind)
    with pytest.raises(TypeError, match="x and b must live in the same memory space"):
        f(x, A, FakeCudaTensor(N))
    with pytest.raises(TypeError, match="x and b must live in the same memory space"):
        f(FakeCudaTensor(N), A, b)
    wide = np.zeros(2 * N, np.complex128)
    if kind == "numpy":
        with pytest.raises(TypeError, match="updated in place"):
            f(wide[::2], A, b)                                          # not contiguous
        with pytest.raises(TypeError, match="updated in place"):
            f(np.zeros(N, np.complex64), A, b)
        with pytest.raises(TypeError, match="updated in place"):
            f([0j] * N, A, b)
        with pytest.raises(ValueError, match="DimensionMismatch: x"):
            f(np.zeros(N + 1, np.complex128), A, b)
        with pytest.raises(ValueError, match="DimensionMismatch: b"):
            f(x, A, np.ones(N - 1, np.complex128))
        f(x, A, [4.0] * N)                                              # b is only read: converted, the copy alive during the call
        assert lib.calls[-1]["px"] == _ptr(x) and lib.calls[-1]["pb"] != _ptr(x) and np.all(lib.calls[-1]["b"] == 4.0)
        assert len(lib.calls) == 1
    else:
        for bad in (torch.from_numpy(wide)[::2], torch.zeros(N, dtype=torch.complex64), torch.zeros(N + 1, dtype=torch.complex128)):
            with pytest.raises(TypeError, match="x: need a contiguous complex128 tensor"):
                f(bad, A, b)
            with pytest.raises(TypeError, match="b: need a contiguous complex128 tensor"):
                f(x, A, bad)
        assert not lib.calls


@pytest.mark.parametrize("name,kind", BATCH)
def test_batch_refusals(lib, name, kind):
    f = getattr(pkg, name)
    X, B = _arrays(name, kind)
    with pytest.raises(TypeError, match="X and B must live in the same memory space"):
        f(FakeCudaTensor(2, N), A, torch.from_numpy(np.ones((2, N), np.complex128)))
    if kind == "numpy":
        for bad in (np.zeros((N, 2), np.complex128).T, np.zeros((2, N)), np.zeros((2, N), np.complex64),
                    np.zeros(2 * N, np.complex128), np.zeros((2, N + 1), np.complex128), [[0j] * N] * 2):
            with pytest.raises(TypeError, match="X must be a C-contiguous complex128 array of shape"):
                f(bad, A, B)
        for bad in (np.ones((3, N), np.complex128), np.ones((2, N - 1), np.complex128), np.ones(2 * N, np.complex128)):
            with pytest.raises(ValueError, match="DimensionMismatch: B"):
                f(X, A, bad)
        Bt = np.arange(2.0 * N).reshape(N, 2).T                         # B is only read: a contiguous complex128 copy goes in
        f(X, A, Bt)
        assert lib.calls[-1]["px"] == _ptr(X) and lib.calls[-1]["pb"] not in (_ptr(X), _ptr(B), Bt.ctypes.data)
        assert np.array_equal(lib.calls[-1]["b"].reshape(2, N), Bt)     # ... and is alive, with its values, during the call
        assert len(lib.calls) == 1
    else:
        with pytest.raises(TypeError, match="X must be contiguous"):
            f(torch.zeros((N, 2), dtype=torch.complex128).T, A, B)
        with pytest.raises(TypeError, match="X: need a contiguous complex128 tensor"):
            f(torch.zeros((2, N), dtype=torch.complex64), A, B)
        # a B of another size: each wrapper keeps its own exception type
        with pytest.raises(ValueError if name == "bicgstabl_batch_" else TypeError):
            f(X, A, torch.ones((3, N), dtype=torch.complex128))
        if name == "bicgstabl_batch_":
            with pytest.raises(ValueError, match="DimensionMismatch: X and B must both be"):
                f(X.reshape(-1), A, B.reshape(-1))
        assert not lib.calls
    assert np.all(np.asarray(X) == 0)
