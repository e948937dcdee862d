"""Host-side mirror of the reference's operator surface for the fast-convolution
path, over the lsfc C ABI (include/lsfc.h).

Names, argument meaning and error behaviour follow the Julia reference
(paths relative to the reference root):

  FastM, FastM3D                      src/FastConvolution.jl:11-27, src/FastConvolution3D.jl:7-26
  M * b, mul_(Y, M, b) (= mul!)       src/FastConvolution.jl:43-54, src/FastConvolution3D.jl:31-37
  size, eltype                        src/FastConvolution.jl:31-41
  fastconvolution, FFTconvolution     src/FastConvolution.jl:58-154, src/FastConvolution3D.jl:39-63
  buildFastConvolution[3D]            src/FastConvolution.jl:170-236, src/FastConvolution3D.jl:68-101
  referenceValsTrapRule               src/FastConvolution.jl:407-415
  sampleGConv / sampleG3D             src/FastConvolution.jl:278-306, src/FastConvolution3D.jl:136-160
  gmres_ (= gmres!)                   IterativeSolvers.jl, call sites examples/example.jl:85,91
  bicgstabl_ (= bicgstabl!)           IterativeSolvers.jl (the short-recurrence alternative; same Pl hook)
  M.T, M.H, M.rmatvec                 transpose(M), M' of LinearMaps / rmatvec of scipy's LinearOperator (lsfc_plan_set_op)
  complex nu, M.nu_is_complex         beyond the reference's nu::Array{Float64,1}: an absorbing medium (lsfc_plan_set_nu_complex)

Vectors are flat complex128 arrays in column-major (x fastest) order: numpy
arrays (host memory, copied through PCIe inside the call) or torch CUDA tensors
(device memory, zero-copy).  All arithmetic runs in HIP kernels; nothing here
computes on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L
from .preconditioner import _op_of as _precond_op_of


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _vec(a, N, name, count=1, plan=None):
    """-> (pointer, memspace, keepalive).  For CUDA tensors the plan is moved onto torch's current stream, so the
    library's kernels are ordered with the caller's torch work (stream 0 == the legacy default stream)."""
    if _is_torch(a):
        import torch
        if a.dtype != torch.complex128 or not a.is_contiguous() or a.numel() != N * count:
            raise TypeError(f"{name}: need a contiguous complex128 tensor with {N * count} entries")
        if a.is_cuda and plan is not None:
            L.check(L.load().lsfc_plan_set_stream(plan, C.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)))
        return C.c_void_p(a.data_ptr()), (L.LSFC_MEM_DEVICE if a.is_cuda else L.LSFC_MEM_HOST), a
    arr = np.ascontiguousarray(a, dtype=np.complex128)
    if arr.size != N * count:
        raise ValueError(f"DimensionMismatch: {name} has {arr.size} entries, operator needs {N * count}")
    return arr.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST, arr


def _nu_array(nu):
    """nu as the plan takes it, flat: a complex dtype stays complex128 (the complex path, even if every imaginary part is 0),
    anything else becomes float64 (the real path)"""
    nu = np.asarray(nu)
    return np.ascontiguousarray(nu, dtype=np.complex128 if np.iscomplexobj(nu) else np.float64).reshape(-1)


def _nu_real_part(nu):
    """what the creators take (they are real: a complex plan is a created plan plus one lsfc_plan_set_nu_complex)"""
    return np.ascontiguousarray(nu.real) if np.iscomplexobj(nu) else nu


def _upload_complex_nu(plan, nu):
    """second half of creating an operator with a complex nu; the plan, which no object owns yet, is destroyed if it fails"""
    if np.iscomplexobj(nu):
        rc = L.load().lsfc_plan_set_nu_complex(plan, nu.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST)
        if rc != 0:
            message = L.load().lsfc_last_error()             # (before the destroy, which may overwrite it)
            L.load().lsfc_plan_destroy(plan)
            raise L.LsfcError(rc, message.decode(errors="replace"))


_QUAD = {"trapezoidal": L.LSFC_QUAD_TRAPEZOIDAL, "Greengard_Vico": L.LSFC_QUAD_GREENGARD_VICO}


@contextlib.contextmanager
def _op_of(M):
    """The plan of M means M.T or M.H while a call through such a view runs, and M again afterwards (also when it raises)"""
    op = getattr(M, "_op", L.LSFC_OP_N)
    if op == L.LSFC_OP_N:
        yield
        return
    lib = L.load()
    L.check(lib.lsfc_plan_set_op(M._plan, op))
    try:
        yield
    finally:
        lib.lsfc_plan_set_op(M._plan, L.LSFC_OP_N)


def _mul_into(M, Y, b):
    """mul!(Y, M, b) for an operator or a view of one"""
    px, sx, kx = _vec(b, M.N, "b", plan=M._plan)
    if _is_torch(Y):
        py, sy, _ = _vec(Y, M.N, "Y")
        if sy != sx:
            raise TypeError("Y and b must live in the same memory space")
    else:
        if not (isinstance(Y, np.ndarray) and Y.dtype == np.complex128 and Y.flags.c_contiguous and Y.size == M.N):
            raise TypeError("Y: need a contiguous complex128 array of the operator size")
        if sx != L.LSFC_MEM_HOST:
            raise TypeError("Y and b must live in the same memory space")
        py = Y.ctypes.data_as(C.c_void_p)
    with _op_of(M):
        L.check(L.load().lsfc_apply(M._plan, px, py, sx))
    return Y


class _Operator:
    """Common behaviour of FastM / FastM3D: owns one lsfc plan."""
    _plan = None

    # -- traits: src/FastConvolution.jl:31-41 --------------------------------
    def size(self, dim=None):
        N = int(self.nu.shape[0])
        return N if dim is not None else ((N,), (N,))      # tuple-of-tuples quirk kept

    @property
    def shape(self):
        N = int(self.nu.shape[0])
        return (N, N)

    def eltype(self):
        return np.complex128

    dtype = np.complex128

    @property
    def N(self):
        return int(L.load().lsfc_plan_size(self._plan))

    @property
    def pipeline(self):
        return L.load().lsfc_plan_pipeline(self._plan).decode()

    @property
    def padded_dims(self):
        d, p = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        L.check(L.load().lsfc_plan_dims(self._plan, d, p))
        return tuple(p)

    def _out_like(self, b, count=1):
        if _is_torch(b):
            import torch
            return torch.empty(self.N * count, dtype=torch.complex128, device=b.device)
        return np.empty(self.N * count, dtype=np.complex128)

    # -- the apply -------------------------------------------------------------
    def __mul__(self, b):
        return fastconvolution(self, b)

    __matmul__ = __mul__
    matvec = __mul__

    def mul_(self, Y, b):
        """LinearAlgebra.mul!(Y, M, b): Y[:] = M*b  (src/FastConvolution.jl:50-54)."""
        return _mul_into(self, Y, b)

    # -- transpose and adjoint (lsfc_plan_set_op): light views, no second plan ---
    def transpose(self):
        """I + omega^2 diag(nu) G: the transpose of M for the symmetric Green's matrix (checked by the library at the first call)"""
        return OperatorView(self, L.LSFC_OP_T)

    def adjoint(self):
        """conj(M.T conj(.)), the adjoint of M (omega is real): b + omega^2 conj(nu) .* conj(G conj(b)), so a complex nu enters
        conjugated"""
        return OperatorView(self, L.LSFC_OP_H)

    T = property(transpose)
    H = property(adjoint)

    def rmatvec(self, b):
        return self.H * b

    def symmetry_defect(self):
        """|sum y.*(G x) - sum x.*(G y)| / (||G x|| ||y||) of two fixed probe vectors through the plan's own convolution
        (lsfc_plan_symmetry_defect); the views exist where it is <= 1e-10"""
        d = C.c_double(0)
        L.check(L.load().lsfc_plan_symmetry_defect(self._plan, C.byref(d)))
        return d.value

    def aslinearoperator(self):
        """scipy.sparse.linalg.LinearOperator with matvec and rmatvec (LSQR, BiCG, QMR) on host vectors"""
        from scipy.sparse.linalg import LinearOperator
        H = self.H
        return LinearOperator(self.shape, matvec=lambda v: self * np.asarray(v).reshape(-1),
                              rmatvec=lambda v: H * np.asarray(v).reshape(-1), dtype=np.complex128)

    def set_nu(self, nu):
        """Replace the contrast.  A real dtype takes the real path (and leaves the complex one, if the plan was on it), a complex
        dtype the complex path (lsfc_plan_set_nu_complex).  A torch CUDA tensor (float64 or complex128) is read on the device; as
        with every device vector handed to an operator, the plan is moved onto torch's current stream first and stays there
        (lsfc_plan_set_stream)."""
        lib = L.load()
        if _is_torch(nu):
            import torch
            if nu.dtype not in (torch.float64, torch.complex128) or not nu.is_contiguous():
                raise TypeError("nu: need a contiguous float64 or complex128 tensor")
            if nu.numel() != self.N:
                raise ValueError("DimensionMismatch: nu")
            entry = lib.lsfc_plan_set_nu_complex if nu.dtype == torch.complex128 else lib.lsfc_plan_set_nu
            if nu.is_cuda:
                L.check(lib.lsfc_plan_set_stream(self._plan, C.c_void_p(torch.cuda.current_stream(nu.device).cuda_stream)))
            L.check(entry(self._plan, C.c_void_p(nu.data_ptr()), L.LSFC_MEM_DEVICE if nu.is_cuda else L.LSFC_MEM_HOST))
            self.nu = nu.detach().cpu().numpy().reshape(-1)
            return
        nu = _nu_array(nu)
        if nu.size != self.N:
            raise ValueError("DimensionMismatch: nu")
        entry = lib.lsfc_plan_set_nu_complex if np.iscomplexobj(nu) else lib.lsfc_plan_set_nu
        L.check(entry(self._plan, nu.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
        self.nu = nu

    @property
    def nu_is_complex(self):
        """whether the plan multiplies by a complex nu (lsfc_plan_nu_is_complex): follows the dtype last given, not its values"""
        flag = C.c_int(0)
        L.check(L.load().lsfc_plan_nu_is_complex(self._plan, C.byref(flag)))
        return bool(flag.value)

    def working_symbol(self):
        """The symbol as the device pipeline stores it (tests / debugging)."""
        cnt = C.c_int64(0)
        L.check(L.load().lsfc_plan_get_symbol(self._plan, None, 0, C.byref(cnt)))
        out = np.empty(cnt.value, dtype=np.complex128)
        L.check(L.load().lsfc_plan_get_symbol(self._plan, out.ctypes.data_as(C.c_void_p), cnt.value, C.byref(cnt)))
        return out

    def set_tuning(self, **knobs):
        """Benchmark knobs of the pruned pipeline (results never depend on them)."""
        for key, value in knobs.items():
            L.check(L.load().lsfc_plan_set_tuning(self._plan, key.encode(), int(value)))

    def describe_passes(self, nrhs=1):
        """The kernels an apply of ``nrhs`` right-hand sides launches under the present tuning (lsfc_plan_describe_passes):
        one line per pass -- family and template flags -- and the storage line (pitches, symbol layout)."""
        need = C.c_int64(0)
        L.check(L.load().lsfc_plan_describe_passes(self._plan, int(nrhs), None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value)
        L.check(L.load().lsfc_plan_describe_passes(self._plan, int(nrhs), buf, need.value, C.byref(need)))
        return buf.value.decode()

    def synchronize(self):
        L.check(L.load().lsfc_plan_synchronize(self._plan))

    def close(self):
        if self._plan is not None:
            L.load().lsfc_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OperatorView:
    """M.T or M.H: the parent operator plus an op, no second plan.  Accepted wherever an operator is (fastconvolution, mul_,
    apply_batch mode 0, the four solvers, time_apply, profile_apply): a call through a view sets the op of the parent's
    plan, calls, and restores M.  conj(M) is not offered, so M.T.H and M.H.T raise."""

    dtype = np.complex128

    def __init__(self, parent, op):
        self.parent, self._op = parent, op

    @property
    def _plan(self):
        return self.parent._plan

    @property
    def N(self):
        return self.parent.N

    @property
    def shape(self):
        return self.parent.shape

    def size(self, dim=None):
        return self.parent.size(dim)

    def eltype(self):
        return np.complex128

    def _out_like(self, b, count=1):
        return self.parent._out_like(b, count)

    def _other(self, op, name):
        if op == self._op:
            return self.parent
        raise NotImplementedError(f"{name}: conj(M) is not offered (only M, M.T and M.H)")

    def transpose(self):
        return self._other(L.LSFC_OP_T, "M.H.T")

    def adjoint(self):
        return self._other(L.LSFC_OP_H, "M.T.H")

    T = property(transpose)
    H = property(adjoint)

    def __mul__(self, b):
        return fastconvolution(self, b)

    __matmul__ = __mul__
    matvec = __mul__

    def mul_(self, Y, b):
        return _mul_into(self, Y, b)


class FastM(_Operator):
    """FastM(GFFT, nu, ne, me, n, m, k; quadRule="trapezoidal") -- src/FastConvolution.jl:11-27.
    GFFT: (ne, me) complex, centred order for Greengard_Vico, FFT order for trapezoidal."""

    def __init__(self, GFFT, nu, ne, me, n, m, k, quadRule="trapezoidal", flags=0, device=0, _plan=None):
        self.GFFT, self.ne, self.me, self.n, self.m = GFFT, int(ne), int(me), int(n), int(m)
        self.omega, self.quadRule = float(k), quadRule
        self.nu = _nu_array(nu)
        if _plan is not None:
            self._plan = _plan
            return
        if quadRule not in _QUAD:
            # the reference fails at apply time with "B not defined" (src/FastConvolution.jl:106)
            raise NameError(f"UndefVarError: B not defined (unknown quadRule {quadRule!r})")
        G = np.asarray(GFFT, dtype=np.complex128)
        if G.shape != (self.ne, self.me):
            raise ValueError(f"DimensionMismatch: GFFT has shape {G.shape}, expected {(self.ne, self.me)}")
        if self.nu.size != self.n * self.m:
            raise ValueError("DimensionMismatch: nu")
        Gf = np.asfortranarray(G)
        plan = C.c_void_p()
        L.check(L.load().lsfc_plan_create_2d(C.byref(plan), self.n, self.m, self.ne, self.me,
                                             _nu_real_part(self.nu).ctypes.data_as(C.c_void_p), Gf.ctypes.data_as(C.c_void_p),
                                             self.omega, _QUAD[quadRule], flags, device))
        _upload_complex_nu(plan, self.nu)
        self._plan = plan


class FastM3D(_Operator):
    """FastM3D(GFFT, nu, ne, me, le, n, m, l, k; quadRule="Greengard_Vico") -- src/FastConvolution3D.jl:7-26."""

    def __init__(self, GFFT, nu, ne, me, le, n, m, l, k, quadRule="Greengard_Vico", flags=0, device=0, _plan=None):
        self.GFFT = GFFT
        self.ne, self.me, self.le, self.n, self.m, self.l = int(ne), int(me), int(le), int(n), int(m), int(l)
        self.omega, self.quadRule = float(k), quadRule
        self.nu = _nu_array(nu)
        if _plan is not None:
            self._plan = _plan
            return
        if quadRule not in _QUAD:
            raise NameError(f"UndefVarError: B not defined (unknown quadRule {quadRule!r})")
        G = np.asarray(GFFT, dtype=np.complex128)
        if G.shape != (self.ne, self.me, self.le):
            raise ValueError(f"DimensionMismatch: GFFT has shape {G.shape}, expected {(self.ne, self.me, self.le)}")
        if self.nu.size != self.n * self.m * self.l:
            raise ValueError("DimensionMismatch: nu")
        Gf = np.asfortranarray(G)
        plan = C.c_void_p()
        L.check(L.load().lsfc_plan_create_3d(C.byref(plan), self.n, self.m, self.l, self.ne, self.me, self.le,
                                             _nu_real_part(self.nu).ctypes.data_as(C.c_void_p), Gf.ctypes.data_as(C.c_void_p),
                                             self.omega, _QUAD[quadRule], flags, device))
        _upload_complex_nu(plan, self.nu)
        self._plan = plan


# ---------------------------------------------------------------------------
# free functions with the reference's names
# ---------------------------------------------------------------------------
def size(M, dim=None):
    return M.size(dim)


def eltype(M):
    return M.eltype()


def fastconvolution(M, b):
    """b + omega^2 * G*(nu .* b)  (src/FastConvolution.jl:58-107; `*` of FastM3D)."""
    px, sx, keep = _vec(b, M.N, "b", plan=M._plan)
    y = M._out_like(keep)
    py, _, _ = _vec(y, M.N, "y")
    with _op_of(M):
        L.check(L.load().lsfc_apply(M._plan, px, py, sx))
    return y


def mul_(Y, M, b):
    """mul!(Y, M, b)."""
    return M.mul_(Y, b)


def FFTconvolution(M, b):
    """Bare convolution (src/FastConvolution.jl:110-154, src/FastConvolution3D.jl:39-63).  As in the
    reference, only the 2D trapezoidal branch multiplies by nu (src/FastConvolution.jl:122 vs :141)."""
    if isinstance(M, FastM) and M.n != M.m:
        # the reference allocates (ne, ne) and crops n in both dimensions (:120,:132): square grids only
        raise ValueError("DimensionMismatch: FFTconvolution(::FastM) assumes n == m")
    apply_nu = 1 if (isinstance(M, FastM) and M.quadRule == "trapezoidal") else 0
    px, sx, keep = _vec(b, M.N, "b", plan=M._plan)
    y = M._out_like(keep)
    py, _, _ = _vec(y, M.N, "y")
    L.check(L.load().lsfc_convolve(M._plan, px, py, apply_nu, sx))
    return y


def referenceValsTrapRule():
    """src/FastConvolution.jl:407-415."""
    x = 2.0 ** (-np.arange(6.0))
    w = np.array([1 - 0.892j, 1 - 1.35j, 1 - 1.79j, 1 - 2.23j, 1 - 2.67j, 1 - 3.11j])
    return x, w


def _grid2d(x, y):
    n, m = len(x), len(y)
    X = np.repeat(np.asarray(x, float)[:, None], m, axis=1).reshape(-1, order="F")
    Y = np.repeat(np.asarray(y, float)[None, :], n, axis=0).reshape(-1, order="F")
    return X, Y


def buildFastConvolution(x, y, h, k, nu, quadRule="trapezoidal", flags=0, device=0):
    """src/FastConvolution.jl:170-236.  ``nu`` is a callable nu(X, Y), real or complex (an absorbing medium); the symbol is
    generated on the device."""
    x, y = np.asarray(x, float), np.asarray(y, float)
    n, m = len(x), len(y)
    X, Y = _grid2d(x, y)
    nuc = _nu_array(nu(X, Y))                    # the dtype given; the creators take its real part, the complex path follows
    nuv = _nu_real_part(nuc)
    plan = C.c_void_p()
    if quadRule == "trapezoidal":
        _, D = referenceValsTrapRule()
        idx = int(round(k * h))                             # D[round(Int, k*h)], 1-based (src/FastConvolution.jl:175-176)
        if not 1 <= idx <= len(D):
            raise IndexError(f"BoundsError: attempt to access {len(D)}-element Vector at index [{idx}] "
                             "(D[round(Int, k*h)], src/FastConvolution.jl:176)")
        D0 = D[idx - 1]
        L.check(L.load().lsfc_plan_create_trap2d(C.byref(plan), n, m, float(x[0]), float(y[0]), float(h), float(k),
                                                 float(D0.real), float(D0.imag), nuv.ctypes.data_as(C.c_void_p), flags, device))
        _upload_complex_nu(plan, nuc)
        return FastM(None, nuc, 2 * n - 1, 2 * m - 1, n, m, k, quadRule="trapezoidal", _plan=plan)
    if quadRule == "Greengard_Vico":
        box = abs(x[-1] - x[0]) + h
        L.check(L.load().lsfc_plan_create_gv2d(C.byref(plan), n, m, float(box), float(k), nuv.ctypes.data_as(C.c_void_p), flags, device))
        _upload_complex_nu(plan, nuc)
        return FastM(None, nuc, 4 * n, 4 * m, n, m, k, quadRule="Greengard_Vico", _plan=plan)
    raise NameError(f"UndefVarError: unknown quadRule {quadRule!r}")


def buildFastConvolution3D(x, y, z, X, Y, Z, h, k, nu, quadRule="Greengard_Vico", flags=0, device=0):
    """src/FastConvolution3D.jl:68-101.  The (4n)^3 symbol is never materialised (137 GB at n=512):
    it is evaluated slab-wise on the device and reduced to the equivalent (2n)^3 grid."""
    if quadRule != "Greengard_Vico":
        raise NameError(f"UndefVarError: unknown quadRule {quadRule!r}")
    x = np.asarray(x, float)
    n, m, l = len(x), len(y), len(z)
    nuc = _nu_array(nu(X, Y, Z) if callable(nu) else nu)
    nuv = _nu_real_part(nuc)
    box = abs(x[-1] - x[0]) + h
    plan = C.c_void_p()
    L.check(L.load().lsfc_plan_create_gv3d(C.byref(plan), n, m, l, float(box), float(k), nuv.ctypes.data_as(C.c_void_p), flags, device))
    _upload_complex_nu(plan, nuc)
    return FastM3D(None, nuc, 4 * n, 4 * m, 4 * l, n, m, l, k, _plan=plan)


def sampleGConv(k, X, Y, indS, fastconv):
    """src/FastConvolution.jl:278-306: one FFTconvolution per delta source (batched on the device)."""
    return _sample(indS, fastconv)


def sampleG3D(k, X, Y, Z, indS, fastconv):
    """src/FastConvolution3D.jl:136-160."""
    return _sample(indS, fastconv)


def _sample(indS, M):
    N, ns = M.N, len(indS)
    out = np.empty((ns, N), dtype=np.complex128)
    if isinstance(M, FastM) and M.quadRule == "trapezoidal":
        # the reference's trapezoidal FFTconvolution multiplies the source by nu (src/FastConvolution.jl:122):
        # keep that quirk literally, one convolution per source
        R = np.zeros((ns, N), dtype=np.complex128)
        for i, ii in enumerate(indS):
            R[i, ii] = 1.0
        L.check(L.load().lsfc_apply_batch(M._plan, R.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), ns, 2, L.LSFC_MEM_HOST))
        return out
    # Greengard-Vico: rows of the Green's matrix = shifted copies of the (even) kernel -> one convolution + gathers
    src = np.ascontiguousarray(indS, dtype=np.int64)
    L.check(L.load().lsfc_sample_sources(M._plan, src.ctypes.data_as(C.c_void_p), ns, out.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST))
    return out


# ---------------------------------------------------------------------------
# GMRES
# ---------------------------------------------------------------------------
class ConvergenceHistory:
    """The part of IterativeSolvers.ConvergenceHistory the reference scripts read."""

    def __init__(self, resnorm, iters, mvps, isconverged):
        self.data = {"resnorm": resnorm}
        self.iters, self.mvps, self.isconverged = iters, mvps, isconverged

    def __getitem__(self, key):
        return self.data[key.lstrip(":")]


class _DevPtr:
    """Minimal __cuda_array_interface__ carrier so torch can alias a raw device pointer (complex128 vector)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<c16", "data": (ptr, False), "version": 2}


def _device_view(ptr, n):
    import torch
    return torch.as_tensor(_DevPtr(ptr, n), device="cuda")


_ORTH = {"ModifiedGramSchmidt": L.LSFC_ORTH_MGS, "ClassicalGramSchmidt": L.LSFC_ORTH_CGS, "DGKS": L.LSFC_ORTH_DGKS}


def _solve_vecs(x, b, A):
    """(x, b) of a single solve -> (px, pb, memspace, keepalive of b); x is updated in place, so it goes in as it is"""
    px, sx, keepx = _vec(x, A.N, "x", plan=A._plan)
    pb, sb, keepb = _vec(b, A.N, "b")
    if sx != sb:
        raise TypeError("x and b must live in the same memory space")
    if not _is_torch(x) and keepx is not x:
        raise TypeError("x must be a contiguous complex128 array (it is updated in place)")
    return px, pb, sx, keepb


def _batch_vecs(X, B, A):
    """(X, B) of a batched solve, one right-hand side per row -> (nrhs, (px, pb, memspace, keepalive of B)); X is
    updated in place, so it goes in as it is"""
    N = A.N
    if _is_torch(X):
        nrhs = X.shape[0]
        px, sx, keepx = _vec(X.reshape(-1), N, "X", count=nrhs, plan=A._plan)
        pb, sb, keepb = _vec(B.reshape(-1), N, "B", count=nrhs)
        if keepx.data_ptr() != X.data_ptr():
            raise TypeError("X must be contiguous (it is updated in place)")
        if sx != sb:
            raise TypeError("X and B must live in the same memory space")
        return nrhs, (px, pb, sx, keepb)
    if not (isinstance(X, np.ndarray) and X.dtype == np.complex128 and X.flags.c_contiguous and X.ndim == 2 and X.shape[1] == N):
        raise TypeError(f"X must be a C-contiguous complex128 array of shape (nrhs, {N}) (it is updated in place)")
    Bc = np.ascontiguousarray(B, dtype=np.complex128)
    if Bc.shape != X.shape:
        raise ValueError("DimensionMismatch: B")
    return X.shape[0], (X.ctypes.data_as(C.c_void_p), Bc.ctypes.data_as(C.c_void_p), L.LSFC_MEM_HOST, Bc)


def _precond_opts(opts, Pl, Pl_on_device, A, x, sx, err):
    """fill precond / precond_user / precond_on_device of a solver's option struct (gmres_ documents the three routes);
    returns what must stay alive for the duration of the call; an exception of Pl ends up in err"""
    native_pc = getattr(Pl, "_pc", None) if Pl is not None else None
    if native_pc is not None:
        # device-resident SparsifyingPreconditioner: the library calls it directly, no Python in the loop; the Krylov
        # basis lives on the device wherever x and b live, so the preconditioner sees device vectors either way
        if sx == L.LSFC_MEM_DEVICE:
            import torch
            Pl.set_stream(torch.cuda.current_stream(x.device).cuda_stream)
        else:
            L.check(L.load().lsfc_plan_set_stream(A._plan, None))
            Pl.set_stream(0)
        opts.precond = C.cast(L.load().lsfc_precond_callback, L.PRECOND_FN)
        opts.precond_user = native_pc
        opts.precond_on_device = 1
        return None
    if Pl is None:
        return None

    def _cb(user, v, n):
        try:
            if Pl_on_device:
                Pl(_device_view(C.cast(v, C.c_void_p).value, n))
                return 0
            Pl(np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_double)), shape=(2 * n,)).view(np.complex128))
            return 0
        except Exception as e:      # never let a Python exception cross the C boundary
            err.append(e)
            return 1
    cb = L.PRECOND_FN(_cb)
    opts.precond = cb
    opts.precond_on_device = 1 if Pl_on_device else 0
    return cb


def _solve(entry, A, x, vecs, nrhs, opts, Pl, Pl_on_device, cap, ok=(0,), status=None):
    """One call of the library's solver `entry` (nrhs None: the single form) -> (rc, results, resnorm rows).  In this order:
    the stream moves of _precond_opts, the call, the exception of the caller's Pl (the library only saw its callback fail),
    the return code.  The copy of b in vecs, r_shadow (the caller holds it) and the ctypes callback live until this returns."""
    px, pb, sx, keepb = vecs
    err = []
    native = getattr(Pl, "_pc", None) is not None
    a_op, p_op = getattr(A, "_op", L.LSFC_OP_N), getattr(Pl, "_op", L.LSFC_OP_N)
    if native and p_op != a_op:
        if p_op == L.LSFC_OP_N:
            raise ValueError("a SparsifyingPreconditioner approximates inv(M), not its transpose or adjoint: not available with M.T / M.H "
                             "(P.T and P.H of a block-tridiagonal one are)")
        names = ("", ".T", ".H")
        raise ValueError(f"Pl = P{names[p_op]} approximates inv(M{names[p_op]}), not inv(M{names[a_op]}): the ops of operator and preconditioner must agree")
    cb = _precond_opts(opts, Pl, Pl_on_device, A, x, sx, err)
    rows = 1 if nrhs is None else max(nrhs, 1)
    res = (L.GmresResult * rows)()
    resnorm = np.zeros((rows, cap), dtype=np.float64)
    args = [A._plan, px, pb]
    if nrhs is not None:
        args.append(nrhs)
    args += [C.byref(opts), resnorm.ctypes.data_as(C.c_void_p), cap, res]
    if status is not None:
        args.append(status.ctypes.data_as(C.c_void_p))
    with _op_of(A), (_precond_op_of(Pl) if native else contextlib.nullcontext()):    # both ops held for the call, restored after
        rc = getattr(L.load(), entry)(*args, sx)
    if err:
        raise err[0]
    if rc not in ok:
        L.check(rc)
    return rc, res, resnorm


def _history(res, resnorm, cap):
    """ConvergenceHistory of one solve from its result struct and its row of resnorm"""
    return ConvergenceHistory(resnorm[:min(res.iters, cap)].copy(), int(res.iters), int(res.mvps), bool(res.converged))


def _gmres_opts(abstol, reltol, restart, maxiter, initially_zero, orth_meth):
    opts = L.GmresOpts()
    opts.restart = int(restart) if restart is not None else 0
    opts.maxiter = int(maxiter) if maxiter is not None else 0
    opts.reltol = float(reltol) if reltol is not None else -1.0
    opts.abstol = float(abstol)
    opts.orth = _ORTH[orth_meth]
    opts.initially_zero = 1 if initially_zero else 0
    return opts


def _gmres_cap(maxiter, N):
    """length of a resnorm row: one entry per iteration"""
    return max(1, min(int(maxiter) if maxiter is not None else N, 1 << 20))


def gmres_(x, A, b, Pl=None, abstol=0.0, reltol=None, restart=None, maxiter=None, log=False,
           initially_zero=False, orth_meth="ModifiedGramSchmidt", Pl_on_device=False):
    """gmres!(x, A, b; Pl, abstol, reltol, restart, maxiter, log, initially_zero, orth_meth).

    ``Pl`` is a callable ``v -> None`` that overwrites the host numpy vector v with Pl \\ v -- the
    two-argument in-place ``ldiv!(Pl, v)`` of src/preconditioner.jl:147-170.  x is updated in place.
    ``Pl_on_device=True``: Pl instead receives a torch CUDA tensor aliasing the Krylov vector on the device (no PCIe
    round trip) and must work on torch's current stream.
    A ``SparsifyingPreconditioner`` is applied by the library itself on the device.  It goes with the operator of its own
    op: ``Pl=P`` with M, ``Pl=P.T`` with M.T, ``Pl=P.H`` with M.H (block-tridiagonal objects); any other pairing raises
    ValueError.  The same holds for bicgstabl_ and the two batch solvers."""
    vecs = _solve_vecs(x, b, A)
    opts = _gmres_opts(abstol, reltol, restart, maxiter, initially_zero, orth_meth)
    cap = _gmres_cap(maxiter, A.N)
    rc, res, resnorm = _solve("lsfc_gmres", A, x, vecs, None, opts, Pl, Pl_on_device, cap, ok=(0, L.LSFC_ENOTCONV))
    if log:
        return x, _history(res[0], resnorm[0], cap)
    return x


def _bicgstabl_opts(l, max_mv_products, abstol, reltol, initially_zero, r_shadow, N, count, sx, xname):
    """-> (opts, keepalive of r_shadow); r_shadow: None or count vectors, flat, in the memory space of x"""
    opts = L.BicgstablOpts()
    opts.l = int(l)
    opts.max_mv_products = int(max_mv_products) if max_mv_products is not None else 0
    opts.reltol = float(reltol) if reltol is not None else -1.0
    opts.abstol = float(abstol)
    opts.initially_zero = 1 if initially_zero else 0
    if r_shadow is None:
        return opts, None
    ps, ss, keeps = _vec(r_shadow, N, "r_shadow", count=count)
    if ss != sx:
        raise TypeError(f"r_shadow and {xname} must live in the same memory space")
    opts.r_shadow = ps
    return opts, keeps


def _bicgstabl_cap(opts, N):
    """length of a resnorm row: one entry per cycle of 2 l operator applications (capped like gmres_)"""
    cap = (opts.max_mv_products if opts.max_mv_products > 0 else N) // (2 * max(opts.l, 1)) + 2
    return max(1, min(cap, 1 << 20))


def bicgstabl_(x, A, b, l=2, Pl=None, max_mv_products=None, abstol=0.0, reltol=None, log=False, Pl_on_device=False,
               r_shadow=None, initially_zero=False):
    """bicgstabl!(x, A, b, l; Pl, max_mv_products, abstol, reltol, log): left-preconditioned BiCGStab(l) on the device
    (lsfc_bicgstabl).  2 l + 3 work vectors whatever the iteration count, where gmres_ keeps restart + 2.

    ``Pl`` as in ``gmres_``: a callable on a host numpy vector, on a torch CUDA tensor (``Pl_on_device=True``), or a
    ``SparsifyingPreconditioner`` (applied by the library on the device, no host code inside the BiCG part).
    Defaults: l = 2 (1..8), reltol sqrt(eps), abstol 0, max_mv_products N.  The history has one residual norm per cycle
    (``iters`` counts cycles of l BiCG steps and one minimal-residual step, 2 l operator applications).
    Departure from IterativeSolvers: the shadow residual is the preconditioned initial residual, not ``rand`` -- or
    ``r_shadow`` (N complex, in the memory space of x), so that a solve is reproducible bit for bit.
    A breakdown (rho, sigma or gamma zero where it divides, or not finite) ends the solve with x the last finite iterate;
    the history then reports ``isconverged == False`` unless that iterate is within the tolerance already.  x is
    updated in place.
    Single-device plans; on a ``MultiDeviceFastM3D`` the library refuses (LsfcError) and ``bicgstabl_multi_`` solves."""
    return _bicgstabl("lsfc_bicgstabl", x, A, b, l, Pl, max_mv_products, abstol, reltol, log, Pl_on_device, r_shadow, initially_zero)


def bicgstabl_multi_(x, A, b, l=2, Pl=None, max_mv_products=None, abstol=0.0, reltol=None, log=False, Pl_on_device=False,
                     r_shadow=None, initially_zero=False):
    """``bicgstabl_`` on a ``MultiDeviceFastM3D`` (lsfc_bicgstabl_multi): the solver for grids whose GMRES basis does not fit even
    spread over the devices.  x, b and r_shadow are host (numpy) vectors of the full size, ``Pl`` is None or a callable on the
    WHOLE host vector, and every device keeps its slab of the 2 l + 3 work vectors (checked against the free memory of each
    device); iterates, history, defaults and breakdown rules are those of ``bicgstabl_``.  Nothing is refused on the Python
    side: device tensors, ``Pl_on_device=True``, a ``SparsifyingPreconditioner`` or a single-device operator raise the
    library's LsfcError.  Its own function, so that ``bicgstabl_`` keeps doing what it did with such an operator."""
    return _bicgstabl("lsfc_bicgstabl_multi", x, A, b, l, Pl, max_mv_products, abstol, reltol, log, Pl_on_device, r_shadow, initially_zero)


def _bicgstabl(entry, x, A, b, l, Pl, max_mv_products, abstol, reltol, log, Pl_on_device, r_shadow, initially_zero):
    vecs = _solve_vecs(x, b, A)
    opts, keeps = _bicgstabl_opts(l, max_mv_products, abstol, reltol, initially_zero, r_shadow, A.N, 1, vecs[2], "x")
    cap = _bicgstabl_cap(opts, A.N)
    rc, res, resnorm = _solve(entry, A, x, vecs, None, opts, Pl, Pl_on_device, cap, ok=(0, L.LSFC_ENOTCONV))
    if log:
        hist = _history(res[0], resnorm[0], cap)
        hist.message = L.load().lsfc_last_error().decode(errors="replace") if rc == L.LSFC_ENOTCONV else ""
        return x, hist
    return x


_BICG_REASON = {L.LSFC_BICG_RHO: "rho is not finite", L.LSFC_BICG_SIGMA: "sigma is zero or not finite",
                L.LSFC_BICG_BETA: "beta = rho / sigma is not finite", L.LSFC_BICG_ALPHA: "alpha = rho / sigma is not finite",
                L.LSFC_BICG_GAMMA: "gamma (singular or non-finite Gram matrix)", L.LSFC_BICG_RESIDUAL: "the residual norm is not finite"}


def bicgstabl_batch_(X, A, B, l=2, Pl=None, max_mv_products=None, abstol=0.0, reltol=None, log=False, Pl_on_device=False,
                     r_shadow=None, initially_zero=False):
    """``bicgstabl_`` for several right-hand sides in lock step (lsfc_bicgstabl_batch): rows of B, solutions in the rows of
    X (contiguous, updated in place; numpy, or torch CUDA tensors).  Every step of a cycle is one launch over the rows
    still running, the operator takes them in groups, and a ``SparsifyingPreconditioner`` takes them in group sweeps; any
    other ``Pl`` is called for one row at a time (a host vector, or a torch CUDA tensor with ``Pl_on_device=True``).
    Each row has its own tolerance and stopping test and its iterates are those of ``bicgstabl_`` on that row alone.
    ``r_shadow``: None or one shadow residual per row, in the memory space of X.  nrhs <= 64; device memory
    nrhs (2 l + 3) vectors.  Returns X or (X, [ConvergenceHistory per row]); ``.message`` of a row that did not converge
    names the reason (max_mv_products, or the scalar of the breakdown) and the cycle.  Single-device plans only: on a
    ``MultiDeviceFastM3D`` the library refuses the batch (LsfcError); ``bicgstabl_multi_`` solves there, one right-hand side at a time."""
    torch_in = _is_torch(X)
    if torch_in and (X.dim() != 2 or tuple(B.shape) != tuple(X.shape)):
        raise ValueError(f"DimensionMismatch: X and B must both be (nrhs, {A.N})")
    nrhs, vecs = _batch_vecs(X, B, A)
    if r_shadow is not None:
        r_shadow = r_shadow.reshape(-1) if torch_in else np.asarray(r_shadow).reshape(-1)
    opts, keeps = _bicgstabl_opts(l, max_mv_products, abstol, reltol, initially_zero, r_shadow, A.N, nrhs, vecs[2], "X")
    cap = _bicgstabl_cap(opts, A.N)
    status = np.zeros((max(nrhs, 1), 2), dtype=np.int64)
    _, res, resnorm = _solve("lsfc_bicgstabl_batch", A, X, vecs, nrhs, opts, Pl, Pl_on_device, cap, status=status)
    if not log:
        return X
    hists = []
    for j in range(nrhs):
        h = _history(res[j], resnorm[j], cap)
        code, cyc = int(status[j, 0]), int(status[j, 1])
        h.status = (code, cyc)
        if code == L.LSFC_BICG_CONVERGED:
            h.message = ""
        elif code == L.LSFC_BICG_MAX_MV:
            h.message = "bicgstabl: max_mv_products reached without convergence"
        else:
            h.message = f"bicgstabl: breakdown in cycle {cyc}: {_BICG_REASON.get(code, code)}; x is the last finite iterate"
        hists.append(h)
    return X, hists


def apply_batch(M, B, mode=0):
    """Rows of B (nrhs, N) through the operator in batched passes (lsfc_apply_batch): mode 0 ``M * b``, 1 bare
    convolution, 2 convolution of nu .* b.  The multi-vector form of src/FastConvolution3D.jl:146-159.
    A view (M.T, M.H) is an operator, not a convolution: mode 0 only."""
    if mode != 0 and getattr(M, "_op", L.LSFC_OP_N) != L.LSFC_OP_N:
        raise ValueError("apply_batch: modes 1 and 2 describe G, which M.T and M.H do not change; pass M")
    if _is_torch(B):
        nrhs = B.shape[0]
        pb, sb, keep = _vec(B.reshape(-1), M.N, "B", count=nrhs, plan=M._plan)
        import torch
        Y = torch.empty_like(keep)
        with _op_of(M):
            L.check(L.load().lsfc_apply_batch(M._plan, pb, C.c_void_p(Y.data_ptr()), nrhs, mode, sb))
        return Y.reshape(nrhs, M.N)
    B = np.ascontiguousarray(B, dtype=np.complex128)
    if B.ndim != 2 or B.shape[1] != M.N:
        raise ValueError(f"DimensionMismatch: B must be (nrhs, {M.N})")
    Y = np.empty_like(B)
    with _op_of(M):
        L.check(L.load().lsfc_apply_batch(M._plan, B.ctypes.data_as(C.c_void_p), Y.ctypes.data_as(C.c_void_p), B.shape[0], mode, L.LSFC_MEM_HOST))
    return Y


def gmres_batch_(X, A, B, Pl=None, abstol=0.0, reltol=None, restart=None, maxiter=None, log=False,
                 initially_zero=False, orth_meth="ModifiedGramSchmidt"):
    """``gmres!`` for several right-hand sides at once (rows of B, solutions in the rows of X, updated in place): the
    solves of tests/plasma_example.jl:160-176 (two incident directions, one after the other in the reference) run in
    lock step, one batched operator application per Arnoldi step.  Each row's iterates are those of ``gmres_`` on that
    row alone.  ``Pl``: a SparsifyingPreconditioner is applied on the device to all unconverged rows at once (one group
    sweep per step for a block-tridiagonal object); any other callable ``v -> None`` gets one host vector at a time, row
    after row, on the calling thread.  The library starts no threads, and the groups of rows are the same in every run.
    Returns X or (X, [ConvergenceHistory per row])."""
    nrhs, vecs = _batch_vecs(X, B, A)
    opts = _gmres_opts(abstol, reltol, restart, maxiter, initially_zero, orth_meth)
    cap = _gmres_cap(maxiter, A.N)
    # a device-resident SparsifyingPreconditioner is called by the library on the device vectors, as in gmres_; the
    # right-hand sides meet at it and a block-tridiagonal object takes their Krylov vectors in one group sweep
    _, res, resnorm = _solve("lsfc_gmres_batch", A, X, vecs, nrhs, opts, Pl, False, cap)
    if log:
        return X, [_history(res[j], resnorm[j], cap) for j in range(nrhs)]
    return X


# ---------------------------------------------------------------------------
# timing helpers used by bench.py (HIP events on the plan's own stream)
# ---------------------------------------------------------------------------
def time_apply(M, x_dev, y_dev, reps):
    px, sx, _ = _vec(x_dev, M.N, "x")
    py, sy, _ = _vec(y_dev, M.N, "y")
    if sx != L.LSFC_MEM_DEVICE or sy != L.LSFC_MEM_DEVICE:
        raise TypeError("time_apply needs device tensors")
    ms = C.c_double(0)
    with _op_of(M):
        L.check(L.load().lsfc_time_apply(M._plan, px, py, int(reps), C.byref(ms)))
    return ms.value


def profile_apply(M, x_dev, y_dev, reps=3):
    """(kernel / stage name, mean ms, algorithmic bytes) of one apply; a multi-device plan profiles on its own staging
    vectors (pass None, None)"""
    px = _vec(x_dev, M.N, "x")[0] if x_dev is not None else None
    py = _vec(y_dev, M.N, "y")[0] if y_dev is not None else None
    names = (C.c_char_p * 16)()
    ms, nb, ns = (C.c_double * 16)(), (C.c_double * 16)(), C.c_int(0)
    with _op_of(M):
        L.check(L.load().lsfc_profile_apply(M._plan, px, py, int(reps), 16, names, ms, nb, C.byref(ns)))
    return [(names[i].decode(), ms[i], nb[i]) for i in range(ns.value)]
