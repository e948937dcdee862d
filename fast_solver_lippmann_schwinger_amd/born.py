"""Linearised scattering over the lsfc C ABI (include/lsfc.h, "linearised scattering"): the Frechet derivative J of the map
nu -> data, its adjoint and the gradient of a least-squares misfit, device-resident.

With M u_s = u_inc_s and the data d_s = -omega^2 R (nu .* u_s) of ``Receivers.scattered_field``:

  B = BornOperator(M, R, U_inc)     solves for the background fields of all sources (lock-step batched solves), keeps them on the device
  B.fields, B.data                  (nsrc, N) torch view of the device fields / (nsrc, nrecv) numpy data
  B * dnu, B.apply(dnu)             J dnu = -omega^2 R M^-T (u_s .* dnu): (nsrc, nrecv); real or complex dnu
  B.H * r, B.adjoint(r, real=...)   J^H r = sum_s -omega^2 conj(u_s .* p_s), M p_s = R^T conj(r_s): N complex, or its real part
  B.misfit(d_obs)                   (1/2 sum |d - d_obs|^2, J^H (d - d_obs)); the gradient is real when M.nu is
  B.update(nu)                      M.set_nu(nu) and a new background
  B.aslinearoperator()              scipy LinearOperator (matvec / rmatvec) for LSQR and Gauss-Newton-CG

Reciprocal mode (``mode="reciprocal"`` or ``B.set_mode("reciprocal")``): one solve per receiver and medium for the receiver fields
V = M^-1 R^T (``B.receiver_fields``), after which B * dnu and B.H * r are contractions of the stored U and V without any solve:
(J dnu)[s, r] = -omega^2 sum_i dnu[i] u_s[i] v_r[i].  It pays when (applies per medium) x nsrc > nrecv, which is the loop of LSQR
and Gauss-Newton-CG; ``born_contract`` is the kernel-level entry.

Vectors follow operators.py: numpy arrays (host memory) or torch CUDA tensors (device memory, zero-copy, ordered on torch's
current stream).  Nothing here computes on the CPU except the scalar misfit of the (small) data.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .operators import ConvergenceHistory, _device_view, _is_torch
from .preconditioner import SparsifyingPreconditioner
from .receivers import Receivers

_SOLVERS = {"gmres": L.LSFC_BORN_GMRES, "bicgstabl": L.LSFC_BORN_BICGSTABL}
_MODES = {"adjoint-state": L.LSFC_BORN_ADJOINT_STATE, "reciprocal": L.LSFC_BORN_RECIPROCAL}


def _mode_of(mode):
    if mode not in _MODES:
        raise ValueError(f"BornOperator: mode must be 'adjoint-state' or 'reciprocal', not {mode!r}")
    return _MODES[mode]


class _BornAdjoint:
    """B.H: the parent object plus the op"""

    dtype = np.complex128

    def __init__(self, parent):
        self.parent = parent

    @property
    def shape(self):
        return self.parent.shape[::-1]

    def __mul__(self, r):
        return self.parent.adjoint(r)

    __matmul__ = __mul__
    matvec = __mul__

    @property
    def H(self):
        return self.parent


class BornOperator:
    """BornOperator(M, R, U_inc, Pl=None, solver="gmres", reltol=1e-8, restart=30, l=2, maxiter=None, chunk=None, mode="adjoint-state")

    M: a FastM / FastM3D (not a view); R: a ``Receivers`` on the same grid and device; U_inc: (nsrc, N) incident fields, numpy or
    torch CUDA; Pl: None or a ``SparsifyingPreconditioner`` (the object itself: the library sets its op to follow the solves and
    puts it back).  ``chunk``: sources solved in lock step (None: the largest that fits, at most 64).  ``mode``: "adjoint-state"
    (one batched solve per apply) or "reciprocal" (one solve per receiver and medium, applies without solves)."""

    dtype = np.complex128

    def __init__(self, M, R, U_inc, Pl=None, solver="gmres", reltol=1e-8, restart=30, l=2, maxiter=None, chunk=None, mode="adjoint-state"):
        if getattr(M, "_op", L.LSFC_OP_N) != L.LSFC_OP_N or not hasattr(M, "set_nu"):
            raise TypeError("BornOperator: M must be the operator itself (FastM / FastM3D), not a view of it")
        if not isinstance(R, Receivers):
            raise TypeError("BornOperator: R must be a Receivers object")
        if Pl is not None and not isinstance(Pl, SparsifyingPreconditioner):
            raise TypeError("BornOperator: Pl must be a SparsifyingPreconditioner (not a view of one, not a callable): "
                            "the library sets its op for the solves on M and M.T")
        if solver not in _SOLVERS:
            raise ValueError(f"BornOperator: solver must be 'gmres' or 'bicgstabl', not {solver!r}")
        if chunk is not None and not 1 <= int(chunk) <= 64:
            raise ValueError("BornOperator: chunk must be in 1..64")
        mode_code = _mode_of(mode)
        self.M, self.R, self.Pl = M, R, Pl
        self.N, self.nrecv = int(M.shape[0]), int(R.nrecv)
        if R.N != self.N:
            raise ValueError(f"DimensionMismatch: the operator has {self.N} grid points, the receivers {R.N}")
        opts = L.BornOpts()
        opts.solver = _SOLVERS[solver]
        opts.restart, opts.l = int(restart), int(l)
        opts.maxiter = int(maxiter) if maxiter is not None else 0
        opts.reltol, opts.abstol = float(reltol), 0.0
        opts.precond = Pl._pc if Pl is not None else None
        opts.chunk = int(chunk) if chunk is not None else 0
        self._b = None
        self.nsrc = 0
        self.history = []
        self.converged = True
        b = C.c_void_p()
        L.check(L.load().lsfc_born_create(C.byref(b), M._plan, R._rc, C.byref(opts)))
        self._b = b
        self.receiver_history = []
        if mode_code != L.LSFC_BORN_ADJOINT_STATE:
            L.check(L.load().lsfc_born_set_mode(b, mode_code))          # no background yet: set_background solves for V
        self.set_background(U_inc)

    # -- traits ---------------------------------------------------------------------
    @property
    def shape(self):
        return (self.nsrc * self.nrecv, self.N)

    def info(self):
        """lsfc_born_info as a dict"""
        out = (C.c_int64 * 8)()
        L.check(L.load().lsfc_born_info(self._b, out, None))
        return dict(zip(("N", "nrecv", "nsrc", "chunk", "solver", "device_bytes", "solves", "mvps"), (int(v) for v in out)))

    def _finish(self, rc):
        """after a call that solved: the per-source history; LSFC_ENOTCONV is a result (the outputs are written), not an exception"""
        self.message = L.load().lsfc_last_error().decode(errors="replace") if rc == L.LSFC_ENOTCONV else ""
        if rc not in (0, L.LSFC_ENOTCONV):
            L.check(rc)
        out = (C.c_int64 * 8)()
        res = (L.GmresResult * max(self.nsrc, 1))()
        L.check(L.load().lsfc_born_info(self._b, out, res))
        self.history = [ConvergenceHistory(np.array([res[s].final_resnorm]), int(res[s].iters), int(res[s].mvps), bool(res[s].converged))
                        for s in range(self.nsrc)]
        self.converged = rc == 0
        info = (C.c_int64 * 4)()
        per = (L.GmresResult * max(self.nrecv, 1))()
        L.check(L.load().lsfc_born_receiver_info(self._b, info, per))
        self.receiver_history = [ConvergenceHistory(np.array([per[r].final_resnorm]), int(per[r].iters), int(per[r].mvps), bool(per[r].converged))
                                 for r in range(self.nrecv)] if info[1] > 0 else []

    # -- the mode -------------------------------------------------------------------------
    @property
    def mode(self):
        m, nbytes = C.c_int(0), C.c_int64(0)
        L.check(L.load().lsfc_born_get_mode(self._b, C.byref(m), C.byref(nbytes)))
        return next(k for k, v in _MODES.items() if v == m.value)

    def set_mode(self, mode):
        """"reciprocal": solve for the receiver fields now (with a background present); "adjoint-state": release them"""
        code = _mode_of(mode)
        rc = L.load().lsfc_born_set_mode(self._b, code)
        self.message = L.load().lsfc_last_error().decode(errors="replace") if rc == L.LSFC_ENOTCONV else ""
        if rc not in (0, L.LSFC_ENOTCONV):
            L.check(rc)
        history, converged = self.history, self.converged
        self._finish(rc)
        self.history, self.converged = history, converged and rc == 0

    def receiver_info(self):
        """lsfc_born_receiver_info and the bytes of V as a dict"""
        info = (C.c_int64 * 4)()
        L.check(L.load().lsfc_born_receiver_info(self._b, info, None))
        m, nbytes = C.c_int(0), C.c_int64(0)
        L.check(L.load().lsfc_born_get_mode(self._b, C.byref(m), C.byref(nbytes)))
        return dict(zip(("nrecv", "solves", "mvps", "first_not_converged", "receiver_field_bytes"), (*(int(v) for v in info), int(nbytes.value))))

    @property
    def receiver_fields(self):
        """(nrecv, N) torch view of V = M^-1 R^T on the device (reciprocal mode; valid until the next set_background / update / set_mode)"""
        p, n = C.c_void_p(), C.c_int64(0)
        L.check(L.load().lsfc_born_receiver_fields(self._b, C.byref(p), C.byref(n)))
        return _device_view(p.value, n.value * self.N).reshape(n.value, self.N)

    def _stream_of(self, t):
        import torch
        L.check(L.load().lsfc_plan_set_stream(self.M._plan, C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)))

    # -- the background -----------------------------------------------------------------
    def set_background(self, U_inc):
        """solve M u_s = u_inc_s for the rows of U_inc; B.fields and B.data follow"""
        lib = L.load()
        if _is_torch(U_inc):
            import torch
            if U_inc.dtype != torch.complex128 or U_inc.dim() != 2 or U_inc.shape[1] != self.N or not U_inc.is_contiguous():
                raise TypeError(f"U_inc: need a contiguous complex128 tensor of shape (nsrc, {self.N})")
            nsrc, ptr = int(U_inc.shape[0]), C.c_void_p(U_inc.data_ptr())
            space = L.LSFC_MEM_DEVICE if U_inc.is_cuda else L.LSFC_MEM_HOST
            if U_inc.is_cuda:
                self._stream_of(U_inc)
        else:
            U_inc = np.ascontiguousarray(U_inc, dtype=np.complex128)
            if U_inc.ndim == 1:
                U_inc = U_inc.reshape(1, -1)
            if U_inc.ndim != 2 or U_inc.shape[1] != self.N:
                raise ValueError(f"DimensionMismatch: U_inc must be (nsrc, {self.N})")
            nsrc, ptr, space = int(U_inc.shape[0]), U_inc.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST
        self._u_inc = U_inc
        self.nsrc = 0
        rc = lib.lsfc_born_set_background(self._b, ptr, nsrc, space)
        if rc in (0, L.LSFC_ENOTCONV):
            self.nsrc = nsrc
        self._finish(rc)

    @property
    def fields(self):
        """(nsrc, N) torch view of the background fields on the device (valid until the next set_background / update)"""
        p, n = C.c_void_p(), C.c_int64(0)
        L.check(L.load().lsfc_born_fields(self._b, C.byref(p), C.byref(n)))
        return _device_view(p.value, n.value * self.N).reshape(n.value, self.N)

    @property
    def data(self):
        """d_s = -omega^2 R (nu .* u_s): (nsrc, nrecv) numpy"""
        d = np.empty((self.nsrc, self.nrecv), dtype=np.complex128)
        L.check(L.load().lsfc_born_data(self._b, d.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
        return d

    # -- J and J^H ------------------------------------------------------------------------
    def _call(self, v, count, is_complex, nout, out_real, op, flags):
        lib = L.load()
        if _is_torch(v):
            import torch
            want = torch.complex128 if is_complex else torch.float64
            if v.dtype != want or not v.is_contiguous() or v.numel() != count:
                raise TypeError(f"need a contiguous {want} tensor with {count} entries")
            out = torch.empty(nout, dtype=torch.float64 if out_real else torch.complex128, device=v.device)
            pv, po = C.c_void_p(v.data_ptr()), C.c_void_p(out.data_ptr())
            space = L.LSFC_MEM_DEVICE if v.is_cuda else L.LSFC_MEM_HOST
            if v.is_cuda:
                self._stream_of(v)
            keep = v
        else:
            keep = np.ascontiguousarray(v, dtype=np.complex128 if is_complex else np.float64).reshape(-1)
            if keep.size != count:
                raise ValueError(f"DimensionMismatch: the vector has {keep.size} entries, the operator needs {count}")
            out = np.empty(nout, dtype=np.float64 if out_real else np.complex128)
            pv, po, space = keep.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST
        rc = lib.lsfc_born_apply(self._b, pv, 1 if is_complex else 0, po, op, flags, space)
        self._finish(rc)
        return out

    @staticmethod
    def _is_complex(v):
        if _is_torch(v):
            return v.is_complex()
        return np.iscomplexobj(v)

    def apply(self, dnu):
        """J dnu: (nsrc, nrecv); dnu real (N doubles) or complex"""
        out = self._call(dnu, self.N, bool(self._is_complex(dnu)), self.nsrc * self.nrecv, False, L.LSFC_OP_N, 0)
        return out.reshape(self.nsrc, self.nrecv)

    def adjoint(self, r, real=False):
        """J^H r: N complex, or its real part (N doubles) with real=True; r: (nsrc, nrecv)"""
        if not _is_torch(r):
            r = np.asarray(r, dtype=np.complex128)
        return self._call(r.reshape(-1), self.nsrc * self.nrecv, True, self.N, bool(real), L.LSFC_OP_H, L.LSFC_BORN_REAL if real else 0)

    def __mul__(self, dnu):
        return self.apply(dnu)

    __matmul__ = __mul__
    matvec = __mul__

    def rmatvec(self, r):
        return self.adjoint(r)

    @property
    def H(self):
        return _BornAdjoint(self)

    @property
    def T(self):
        raise NotImplementedError("B.T is not offered: J^T r = conj(J^H conj(r))")

    def misfit(self, d_obs):
        """(phi, grad) with phi = 1/2 sum |d - d_obs|^2 and grad = J^H (d - d_obs): its real part (N doubles) when M.nu is real"""
        res = self.data - np.asarray(d_obs, dtype=np.complex128).reshape(self.nsrc, self.nrecv)
        return 0.5 * float(np.vdot(res, res).real), self.adjoint(res, real=not self.M.nu_is_complex)

    def update(self, nu):
        """M.set_nu(nu) and a new background for the same incident fields"""
        self.M.set_nu(nu)
        self.set_background(self._u_inc)

    def aslinearoperator(self):
        """scipy.sparse.linalg.LinearOperator (nsrc nrecv x N) on host vectors: matvec = J, rmatvec = J^H"""
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=lambda v: self.apply(np.asarray(v).reshape(-1)).reshape(-1),
                              rmatvec=lambda v: self.adjoint(np.asarray(v).reshape(-1)), dtype=np.complex128)

    def close(self):
        if getattr(self, "_b", None) is not None:
            L.load().lsfc_born_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def born_contract(M, U, V, x, op="N", scale=1.0, real=False, accumulate=None):
    """lsfc_born_contract on the grid, device and stream of M (a FastM / FastM3D): U (nsrc, N), V (nrecv, N) complex.
    op="N": x is N real or complex, the result (nsrc, nrecv) with out[s, r] = scale sum_i x[i] U[s, i] V[r, i].
    op="H": x is (nsrc, nrecv) complex, the result N complex (N doubles = its real part with real=True):
    out[i] = accumulate[i] + conj(scale) sum_s conj(U[s, i]) sum_r conj(V[r, i]) x[s, r].
    All of U, V, x (and accumulate) numpy arrays, or all torch CUDA tensors (zero-copy, ordered on torch's current stream)."""
    if op not in ("N", "H"):
        raise ValueError("born_contract: op must be 'N' or 'H'")
    if op == "N" and (real or accumulate is not None):
        raise ValueError("born_contract: real and accumulate go with op='H'")
    lib = L.load()
    N = int(M.shape[0])
    scale = complex(scale)
    flags = (L.LSFC_BORN_REAL if real else 0) | (L.LSFC_BORN_ACCUMULATE if accumulate is not None else 0)
    code = L.LSFC_OP_N if op == "N" else L.LSFC_OP_H
    if _is_torch(U):
        import torch
        for t in (U, V):
            if t.dtype != torch.complex128 or t.dim() != 2 or t.shape[1] != N or not t.is_contiguous() or not t.is_cuda:
                raise TypeError(f"born_contract: U and V must be contiguous complex128 CUDA tensors of shape (members, {N})")
        nsrc, nrecv = int(U.shape[0]), int(V.shape[0])
        x_complex = bool(x.is_complex()) if op == "N" else True
        want = torch.complex128 if x_complex else torch.float64
        if not _is_torch(x) or x.dtype != want or not x.is_contiguous() or not x.is_cuda or x.numel() != (N if op == "N" else nsrc * nrecv):
            raise TypeError("born_contract: x must be a contiguous CUDA tensor of N entries (op='N') or nsrc x nrecv complex entries (op='H')")
        if op == "N":
            out = torch.empty((nsrc, nrecv), dtype=torch.complex128, device=U.device)
        elif accumulate is not None:
            out = accumulate.clone()
            if out.dtype != (torch.float64 if real else torch.complex128) or out.numel() != N or not out.is_cuda:
                raise TypeError("born_contract: accumulate must match the result")
        else:
            out = torch.empty(N, dtype=torch.float64 if real else torch.complex128, device=U.device)
        L.check(lib.lsfc_plan_set_stream(M._plan, C.c_void_p(torch.cuda.current_stream(U.device).cuda_stream)))
        ptr = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
        L.check(lib.lsfc_born_contract(M._plan, ptr(U), nsrc, ptr(V), nrecv, ptr(x), 1 if x_complex else 0, ptr(out), code, flags,
                                       scale.real, scale.imag, L.LSFC_MEM_DEVICE))
        return out
    U, V = (np.ascontiguousarray(a, dtype=np.complex128) for a in (U, V))
    if U.ndim != 2 or V.ndim != 2 or U.shape[1] != N or V.shape[1] != N:
        raise ValueError(f"DimensionMismatch: U and V must be (members, {N})")
    nsrc, nrecv = U.shape[0], V.shape[0]
    x_complex = bool(np.iscomplexobj(x)) if op == "N" else True
    x = np.ascontiguousarray(x, dtype=np.complex128 if x_complex else np.float64).reshape(-1)
    if x.size != (N if op == "N" else nsrc * nrecv):
        raise ValueError("DimensionMismatch: x must have N entries (op='N') or nsrc x nrecv entries (op='H')")
    if op == "N":
        out = np.empty((nsrc, nrecv), dtype=np.complex128)
    elif accumulate is not None:
        out = np.array(accumulate, dtype=np.float64 if real else np.complex128).reshape(-1)
        if out.size != N:
            raise ValueError("DimensionMismatch: accumulate must have N entries")
    else:
        out = np.empty(N, dtype=np.float64 if real else np.complex128)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)            # noqa: E731
    L.check(lib.lsfc_born_contract(M._plan, ptr(U), nsrc, ptr(V), nrecv, ptr(x), 1 if x_complex else 0, ptr(out), code, flags,
                                   scale.real, scale.imag, L.LSFC_MEM_HOST))
    return out
