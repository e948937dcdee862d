"""Off-grid sources and receivers over the lsfc C ABI (include/lsfc.h, "off-grid sources and receivers").

The reference's drivers build the incident field on the host and stop at the total field on the grid
(examples/example3D.jl:46-50, :78-81).  ``Receivers`` is the dense nrecv x N sampling operator R between grid vectors and
receivers off the grid -- point receivers, or far-field directions -- with its transpose and adjoint, applied by HIP
kernels without ever forming R:

  R * q, R.T * w, R.H * w         lsfc_receivers_apply with LSFC_OP_N / _T / _H
  R.apply_batch(Q, op="N")        the same on the rows of Q
  R.scattered_field(M, u)         -omega^2 R (nu .* u): the scattered field at the receivers for the total field u
  R.adjoint_source(M, w)          -omega^2 conj(nu) .* (R^H w): the adjoint source of a misfit at the receivers
  R.point_sources(a)              R^T a: the incident field of point sources of amplitudes a
  R.plane_waves(a)                far field only: sum_r a_r exp(i k theta_r . x), rows of B for gmres_batch_

Vectors follow operators.py: numpy arrays (host memory) or torch CUDA tensors (device memory, zero-copy, ordered on
torch's current stream).  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from .operators import _is_torch, _vec

_OPS = {"N": L.LSFC_OP_N, "T": L.LSFC_OP_T, "H": L.LSFC_OP_H, L.LSFC_OP_N: L.LSFC_OP_N, L.LSFC_OP_T: L.LSFC_OP_T,
        L.LSFC_OP_H: L.LSFC_OP_H}


def _axis(v, name):
    """-> (first point, spacing or None for a single point, count); uniform spacing is checked"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size < 1:
        raise ValueError(f"{name}: empty axis")
    if v.size == 1:
        return float(v[0]), None, 1
    d = np.diff(v)
    if not np.all(np.abs(d - d[0]) <= 1e-10 * abs(d[0])) or d[0] <= 0:
        raise ValueError(f"{name}: the axis is not uniformly spaced and increasing")
    return float(v[0]), float((v[-1] - v[0]) / (v.size - 1)), int(v.size)


class _ReceiversView:
    """R.T or R.H: the parent object plus an op"""

    dtype = np.complex128

    def __init__(self, parent, op):
        self.parent, self._op = parent, op

    @property
    def shape(self):
        return self.parent.shape[::-1]

    def __mul__(self, w):
        return self.parent.apply(w, op=self._op)

    __matmul__ = __mul__
    matvec = __mul__


class Receivers:
    """Receivers(x, y, z=None, k=..., points=None, directions=None, device=0)

    x, y[, z]: the axis vectors handed to buildFastConvolution[3D] (uniform, the same spacing h on every axis); the grid
    points are origin + h (ix, iy[, iz]), x fastest.  Exactly one of ``points`` (nrecv, ndim) -- positions off the grid --
    and ``directions`` (nrecv, ndim) -- unit vectors, the far-field pattern -- selects the kind of row."""

    dtype = np.complex128

    def __init__(self, x, y, z=None, k=None, points=None, directions=None, device=0):
        if k is None:
            raise TypeError("Receivers: the wavenumber k is required")
        if (points is None) == (directions is None):
            raise ValueError("Receivers: give exactly one of points= and directions=")
        axes = [_axis(x, "x"), _axis(y, "y")] + ([_axis(z, "z")] if z is not None else [])
        hs = [a[1] for a in axes if a[1] is not None]
        if not hs:
            raise ValueError("Receivers: at least one axis needs two points (h is derived from the axes)")
        if any(abs(hh - hs[0]) > 1e-10 * hs[0] for hh in hs):
            raise ValueError("Receivers: the axes differ in spacing")
        self.ndim = len(axes)
        self.h, self.k = hs[0], float(k)
        self.dims = tuple(a[2] for a in axes)
        self.origin = tuple(a[0] for a in axes)
        self.kind = L.LSFC_RECV_POINTS if points is not None else L.LSFC_RECV_FARFIELD
        c = np.ascontiguousarray(points if points is not None else directions, dtype=np.float64)
        if c.ndim == 1:
            c = c.reshape(1, -1)
        if c.ndim != 2 or c.shape[1] != self.ndim:
            raise ValueError(f"Receivers: coordinates must be (nrecv, {self.ndim})")
        self.coords = c
        self.nrecv = int(c.shape[0])
        self.N = int(np.prod(self.dims))
        self.device = int(device)
        dims = (C.c_int64 * 3)(*(list(self.dims) + [1] * (3 - self.ndim)))
        origin = (C.c_double * 3)(*(list(self.origin) + [0.0] * (3 - self.ndim)))
        rc = C.c_void_p()
        L.check(L.load().lsfc_receivers_create(C.byref(rc), self.ndim, dims, origin, self.h, self.k, self.kind,
                                               c.ctypes.data_as(C.c_void_p), self.nrecv, self.device))
        self._rc = rc

    # -- traits -------------------------------------------------------------------
    @property
    def shape(self):
        return (self.nrecv, self.N)

    def info(self):
        """lsfc_receivers_info as a dict: N, nrecv, receivers per thread of the forward kernel, receivers per LDS chunk of
        the T / H kernel, members per group, bytes of the tables"""
        out = (C.c_int64 * 6)()
        L.check(L.load().lsfc_receivers_info(self._rc, out))
        return dict(zip(("N", "nrecv", "receivers_per_thread", "chunk", "members_per_group", "table_bytes"), (int(v) for v in out)))

    # -- the apply ------------------------------------------------------------------
    def _run(self, v, op, count, M):
        op = _OPS[op]
        nin, nout = (self.N, self.nrecv) if op == L.LSFC_OP_N else (self.nrecv, self.N)
        lib = L.load()
        pv, space, keep = _vec(v, nin, "vector", count=count)
        plan = None
        if M is not None:
            plan = getattr(M, "parent", M)._plan             # a view's medium is its parent's; the plan's op is not read
        if _is_torch(keep):
            import torch
            out = torch.empty(nout * count, dtype=torch.complex128, device=keep.device)
            po = C.c_void_p(out.data_ptr())
            if keep.is_cuda:                                 # ordered with the caller's torch work, like a plan under _vec
                L.check(lib.lsfc_receivers_set_stream(self._rc, C.c_void_p(torch.cuda.current_stream(keep.device).cuda_stream)))
        else:
            out = np.empty(nout * count, dtype=np.complex128)
            po = out.ctypes.data_as(C.c_void_p)
        L.check(lib.lsfc_receivers_apply(self._rc, plan, pv, po, count, op, space))
        return out

    def apply(self, v, op="N", M=None):
        """one vector through R (op "N"), R^T ("T") or R^H ("H"); with M the medium of that operator is fused in"""
        return self._run(v.reshape(-1) if hasattr(v, "reshape") else v, op, 1, M)

    def apply_batch(self, Q, op="N", M=None):
        """the rows of Q (nrhs, N) or (nrhs, nrecv) through R, R^T or R^H; groups of up to 8 rows share one pass"""
        if not _is_torch(Q):
            Q = np.ascontiguousarray(Q, dtype=np.complex128)
        if Q.ndim != 2:
            raise ValueError("apply_batch: Q must be (nrhs, length)")
        nrhs = int(Q.shape[0])
        return self._run(Q.reshape(-1), op, nrhs, M).reshape(nrhs, -1)

    def __mul__(self, q):
        return self.apply(q, "N")

    __matmul__ = __mul__
    matvec = __mul__

    def transpose(self):
        return _ReceiversView(self, L.LSFC_OP_T)

    def adjoint(self):
        return _ReceiversView(self, L.LSFC_OP_H)

    T = property(transpose)
    H = property(adjoint)

    def rmatvec(self, w):
        return self.apply(w, "H")

    def aslinearoperator(self):
        """scipy.sparse.linalg.LinearOperator with matvec and rmatvec on host vectors"""
        from scipy.sparse.linalg import LinearOperator
        return LinearOperator(self.shape, matvec=lambda v: self.apply(np.asarray(v).reshape(-1), "N"),
                              rmatvec=lambda v: self.apply(np.asarray(v).reshape(-1), "H"), dtype=np.complex128)

    # -- both ends of a scattering computation ---------------------------------------
    def scattered_field(self, M, u_total):
        """-omega^2 R (nu .* u_total): the scattered field at the receivers (the far-field pattern on a far-field object)"""
        return self.apply(u_total, "N", M=M)

    def adjoint_source(self, M, w):
        """-omega^2 conj(nu) .* (R^H w): what a residual w at the receivers puts on the grid"""
        return self.apply(w, "H", M=M)

    def point_sources(self, a):
        """R^T a: the field on the grid of point sources of amplitudes a at the receivers' positions (times h^d)"""
        return self.apply(a, "T")

    def plane_waves(self, a):
        """sum_r a_r exp(i k theta_r . x) on the grid: R^H (a / (conj(c_d) h^d)) of a far-field object"""
        if self.kind != L.LSFC_RECV_FARFIELD:
            raise ValueError("plane_waves needs a far-field object (directions=)")
        cd = 1.0 / (4.0 * np.pi) if self.ndim == 3 else np.exp(0.25j * np.pi) / np.sqrt(8.0 * np.pi * self.k)
        scale = 1.0 / (np.conj(cd) * self.h ** self.ndim)
        return self.apply(a * scale, "H")

    def close(self):
        if getattr(self, "_rc", None) is not None:
            L.load().lsfc_receivers_destroy(self._rc)
            self._rc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
