"""Device-resident apply of the reference's SparsifyingPreconditioner (src/preconditioner.jl:27-58, 132-170):

    P = SparsifyingPreconditioner(Msp, As)        # MspInv = lu(Msp) on the host      (:35)
    ldiv!(P, b):  b[:] = MspInv \\ (As * b)        # once per Arnoldi step             (:132-170)

The sparse LU stays on the host, as in the reference (UMFPACK there; scipy's SuperLU here -- any LU of Msp gives
the same operator).  Its factors and As are uploaded once; `ldiv_` then runs entirely on the device (csrc/precond.hip:
CSR SpMV + the two level-scheduled sparse triangular solves of csrc/trisolve.hip, replayed from one hipGraph), so under `gmres_` the Krylov
vector never crosses PCIe.  Msp / As are assembled on the device by sparsify.py (src/SparsifyingMatrix*.jl).

A second route factorises on the device as well (csrc/blocktri_factor.hip, lsfc_precond_create_blocktri): with the slowest grid
axis as block index Msp is block tridiagonal, and exact block elimination with dense explicit inverses of the Schur
blocks replaces the sparse LU.  `SparsifyingPreconditioner(Msp, As, factor="blocktri", nblocks=...)` takes host
matrices; `SparsifyingPreconditioner.from_operator(M)` assembles and factorises from the plan of a FastM / FastM3D
without the matrices ever leaving the device (examples/example3D.jl:57-68 in one call).  ``inverse_dtype="complex64"``
keeps the dense inverses as float pairs (half the memory and half the bytes per apply): the factorisation is the fp64
one, each inverse is rounded once when it is stored, and the applies widen on load and sum in fp64.  ``pivoting="partial"``
inverts every Schur block with partial row pivoting (``"auto"``: only after the pivot-free factorisation broke down); the
stored blocks are the inverses themselves either way, so the applies do not change."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L


# lsfc_precond_schedule's ten counts (include/lsfc.h), in order
SCHEDULE_FIELDS = ("level8", "level16", "level32", "level64", "chains", "chain_groups", "heavy_groups", "run_pieces",
                   "run_max", "run_min")
# lsfc_precond_blocktri_info's six counts, in order
BLOCKTRI_FIELDS = ("blocks", "block_size", "factor_bytes", "launches", "factor_us", "pivoting")
# lsfc_precond_batch_info's four counts, in order
BATCH_FIELDS = ("sweeps", "vectors", "largest_group", "work_bytes")
# inverse_dtype -> LSFC_PRECOND_INV_*
INVERSE_DTYPES = {"complex128": L.LSFC_PRECOND_INV_F64, "complex64": L.LSFC_PRECOND_INV_F32}


def _inverse_precision(inverse_dtype):
    if not isinstance(inverse_dtype, str) or inverse_dtype not in INVERSE_DTYPES:
        raise ValueError(f"inverse_dtype must be 'complex128' or 'complex64', not {inverse_dtype!r}")
    return INVERSE_DTYPES[inverse_dtype]


# pivoting -> LSFC_PRECOND_PIVOT_*
PIVOTING = {"none": L.LSFC_PRECOND_PIVOT_NONE, "partial": L.LSFC_PRECOND_PIVOT_PARTIAL, "auto": L.LSFC_PRECOND_PIVOT_AUTO}


def _pivoting(pivoting):
    if not isinstance(pivoting, str) or pivoting not in PIVOTING:
        raise ValueError(f"pivoting must be 'none', 'partial' or 'auto', not {pivoting!r}")
    return PIVOTING[pivoting]


def _csr_arrays(A):
    A = A.tocsr()
    A.sort_indices()
    return (np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64),
            np.ascontiguousarray(A.data, dtype=np.complex128))


class SparsifyingPreconditioner:
    """SparsifyingPreconditioner(Msp, As; solverType="UMFPACK") -- src/preconditioner.jl:27-58.
    Msp, As: scipy.sparse matrices (N x N, complex).  ``lu``: optional pre-computed scipy.sparse.linalg.SuperLU of Msp.
    ``factor``: "host" (default) -- sparse LU of Msp on the host, level-scheduled triangular solves on the device;
    "blocktri" -- block-tridiagonal factorisation on the device with ``nblocks`` blocks (the slowest grid axis: m in 2D,
    l in 3D); Msp and As must share one pattern, as the pair of `sparsifying_pair` does.
    ``inverse_dtype`` (factor="blocktri" only): "complex128" (default) or "complex64", the storage of the dense inverses
    S_k^{-1}; the factorisation and the sums of the apply are fp64 either way.
    ``pivoting`` (factor="blocktri" only): "none" (default), "partial" -- partial row pivoting inside every Schur block --
    or "auto" -- without pivoting first and, after a breakdown, the whole factorisation again with "partial"."""

    def __init__(self, Msp, As, solverType="UMFPACK", device=0, lu=None, factor="host", nblocks=None, inverse_dtype="complex128",
                 pivoting="none"):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        if solverType not in ("UMFPACK", "MKLPARDISO"):
            raise NameError(f"UndefVarError: unknown solverType {solverType!r}")
        if factor not in ("host", "blocktri"):
            raise ValueError(f"factor must be 'host' or 'blocktri', not {factor!r}")
        precision = _inverse_precision(inverse_dtype)
        if factor == "host" and precision != L.LSFC_PRECOND_INV_F64:
            raise ValueError("inverse_dtype='complex64' needs factor='blocktri': the host LU keeps no dense inverses")
        pivot = _pivoting(pivoting)
        if factor == "host" and pivot != L.LSFC_PRECOND_PIVOT_NONE:
            raise ValueError(f"pivoting={pivoting!r} needs factor='blocktri': the host LU pivots on its own")
        Msp = sp.csc_matrix(Msp, dtype=np.complex128)
        As = sp.csr_matrix(As, dtype=np.complex128)
        N = Msp.shape[0]
        if Msp.shape != (N, N) or As.shape != (N, N):
            raise ValueError("DimensionMismatch: Msp and As must be square and of the same size")
        self.Msp, self.As, self.solverType, self.N = Msp, As, solverType, N
        self.factor = factor
        if factor == "blocktri":
            if nblocks is None:
                raise ValueError("factor='blocktri' needs nblocks (the slowest grid axis)")
            if lu is not None:
                raise ValueError("factor='blocktri' factorises on the device: lu does not apply")
            a_ptr, a_col, a_val = _csr_arrays(As)
            m_ptr, m_col, m_val = _csr_arrays(Msp)
            if not (np.array_equal(a_ptr, m_ptr) and np.array_equal(a_col, m_col)):
                raise ValueError("factor='blocktri': Msp and As must share one sparsity pattern (every stencil entry stored)")
            pc = C.c_void_p()
            p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
            opts = L.BlocktriOpts(inverse_precision=precision, pivoting=pivot)
            L.check(L.load().lsfc_precond_create_blocktri_opts(C.byref(pc), N, int(nblocks), p(m_ptr), p(m_col), p(a_val), p(m_val),
                                                               L.LSFC_MEM_HOST, int(device), C.byref(opts)))
            self._pc = pc
            return
        if lu is None:
            lu = spla.splu(Msp)                      # Pr * Msp * Pc = L * U, no row scaling
        # scipy: Pr Msp Pc = L U with row i of Msp -> row perm_r[i] of L U, column j of Msp -> column perm_c[j] of L U;
        # the C ABI wants the inverse maps (row / column of Msp behind row / column k of L U)
        row_gather = np.empty(N, dtype=np.int64)
        row_gather[np.asarray(lu.perm_r, dtype=np.int64)] = np.arange(N, dtype=np.int64)
        col_scatter = np.empty(N, dtype=np.int64)
        col_scatter[np.asarray(lu.perm_c, dtype=np.int64)] = np.arange(N, dtype=np.int64)
        a_ptr, a_col, a_val = _csr_arrays(As)
        l_ptr, l_col, l_val = _csr_arrays(lu.L)
        u_ptr, u_col, u_val = _csr_arrays(lu.U)
        self.nnz_L, self.nnz_U = int(l_val.size), int(u_val.size)
        pc = C.c_void_p()
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        L.check(L.load().lsfc_precond_create(C.byref(pc), N, p(a_ptr), p(a_col), p(a_val), p(l_ptr), p(l_col), p(l_val),
                                             p(u_ptr), p(u_col), p(u_val), p(row_gather), p(col_scatter), None, int(device)))
        self._pc = pc

    @classmethod
    def from_operator(cls, M, inverse_dtype="complex128", pivoting="none"):
        """The preconditioner of a FastM / FastM3D in one device call (lsfc_precond_create_from_plan): As and
        Msp = As + k^2 AG diag(nu) are assembled into device memory from the plan's kernel, nu and k, and factorised
        there with the slowest axis as block index.  ``Msp`` / ``As`` of the object are None: nothing is downloaded.
        ``inverse_dtype``: storage of the dense inverses, ``pivoting``: "none", "partial" or "auto", as in the constructor."""
        opts = L.BlocktriOpts(inverse_precision=_inverse_precision(inverse_dtype), pivoting=_pivoting(pivoting))
        self = cls.__new__(cls)
        pc = C.c_void_p()
        L.check(L.load().lsfc_precond_create_from_plan_opts(C.byref(pc), M._plan, C.byref(opts)))
        self._pc = pc
        self.Msp = self.As = None
        self.solverType, self.factor = "UMFPACK", "blocktri"
        self.N = int(self.blocktri_info()["blocks"] * self.blocktri_info()["block_size"])
        return self

    @property
    def inverse_dtype(self):
        """storage of the dense inverses of a block-tridiagonal object (lsfc_precond_inverse_precision): "complex128" or
        "complex64"; None on an object of the host-LU route, which keeps none"""
        if self.factor != "blocktri":
            return None
        prec = C.c_int(-1)
        L.check(L.load().lsfc_precond_inverse_precision(self._pc, C.byref(prec)))
        return {v: k for k, v in INVERSE_DTYPES.items()}[prec.value]

    def blocktri_info(self):
        """lsfc_precond_blocktri_info as a dict (BLOCKTRI_FIELDS and min_pivot_ratio)"""
        out = (C.c_int64 * len(BLOCKTRI_FIELDS))()
        ratio = C.c_double(0.0)
        L.check(L.load().lsfc_precond_blocktri_info(self._pc, out, C.byref(ratio)))
        info = dict(zip(BLOCKTRI_FIELDS, (int(v) for v in out)))
        info["min_pivot_ratio"] = ratio.value
        return info

    def blocktri_block(self, k):
        """S_k^{-1} (b x b) of a block-tridiagonal object as stored, widened to complex128 at float storage
        (lsfc_precond_blocktri_get_block; debugging and tests)"""
        b = self.blocktri_info()["block_size"]
        out = np.empty(b * b, dtype=np.complex128)
        L.check(L.load().lsfc_precond_blocktri_get_block(self._pc, int(k), out.ctypes.data_as(C.c_void_p), b * b))
        return out.reshape((b, b), order="F")

    def blocktri_pivots(self, k):
        """perm of block k of a block-tridiagonal object (lsfc_precond_blocktri_get_pivots): perm[i] = row of S_k that became
        pivot row i; the identity on an object factorised without pivoting"""
        b = self.blocktri_info()["block_size"]
        out = np.empty(b, dtype=np.int64)
        L.check(L.load().lsfc_precond_blocktri_get_pivots(self._pc, int(k), out.ctypes.data_as(C.c_void_p), b))
        return out

    # -- P.T / P.H: the preconditioner of M.T / M.H ----------------------------------------------------------------------
    def transpose(self):
        """As^T Msp^-T, which approximates inv(M.T) (block-tridiagonal objects; lsfc_precond_set_op)"""
        return PreconditionerView(self, L.LSFC_OP_T)

    def adjoint(self):
        """conj(P.T conj(.)), which approximates inv(M.H)"""
        return PreconditionerView(self, L.LSFC_OP_H)

    T = property(transpose)
    H = property(adjoint)

    # -- ldiv!(P, b) / P \\ b -- src/preconditioner.jl:132-170 ---------------------------------------------------------
    def ldiv_(self, v):
        """in place: v <- Msp^{-1} (As v).  numpy vector (copied over PCIe) or torch CUDA tensor (stays on the device,
        enqueued on torch's current stream)."""
        from .operators import _vec, _is_torch
        pv, space, keep = _vec(v, self.N, "v")
        if not _is_torch(v) and keep is not v:
            raise TypeError("v must be a contiguous complex128 array (it is updated in place)")
        if space == L.LSFC_MEM_DEVICE:
            import torch
            self.set_stream(torch.cuda.current_stream(v.device).cuda_stream)
        L.check(L.load().lsfc_precond_apply(self._pc, pv, space))
        return v

    def __call__(self, v):                           # usable as the Pl callable of gmres_
        self.ldiv_(v)

    def solve(self, b):
        """P \\ b (out of place)"""
        from .operators import _is_torch
        v = b.clone() if _is_torch(b) else np.array(b, dtype=np.complex128)
        return self.ldiv_(v)

    # -- several right-hand sides at once (lsfc_precond_apply_batch) -----------------------------------------------------
    def ldiv_batch_(self, V):
        """in place: every row of V (nrhs, N) <- Msp^{-1} (As row).  numpy array (staged over PCIe) or torch CUDA tensor
        (stays on the device, enqueued on torch's current stream).  A block-tridiagonal object takes groups of up to 8 rows
        through one sweep that reads every S_k^{-1} once per group; a row's result does not depend on the other rows.
        An object of the host-LU route applies row by row: the bits of `ldiv_` per row."""
        from .operators import _is_torch
        if _is_torch(V):
            import torch
            if V.dtype != torch.complex128 or V.dim() != 2 or V.shape[1] != self.N or V.shape[0] < 1 or not V.is_contiguous():
                raise TypeError(f"V: need a contiguous complex128 tensor of shape (nrhs >= 1, {self.N}), not {tuple(V.shape)} {V.dtype}")
            space = L.LSFC_MEM_DEVICE if V.is_cuda else L.LSFC_MEM_HOST
            if V.is_cuda:
                self.set_stream(torch.cuda.current_stream(V.device).cuda_stream)
            pv = C.c_void_p(V.data_ptr())
        else:
            if not (isinstance(V, np.ndarray) and V.dtype == np.complex128 and V.flags.c_contiguous):
                raise TypeError("V must be a C-contiguous complex128 array (it is updated in place)")
            if V.ndim != 2 or V.shape[1] != self.N or V.shape[0] < 1:
                raise ValueError(f"DimensionMismatch: V has shape {V.shape}, need (nrhs >= 1, {self.N})")
            space, pv = L.LSFC_MEM_HOST, V.ctypes.data_as(C.c_void_p)
        L.check(L.load().lsfc_precond_apply_batch(self._pc, pv, int(V.shape[0]), space))
        return V

    def solve_batch(self, B):
        """rows of P \\ B (out of place)"""
        from .operators import _is_torch
        V = B.clone().contiguous() if _is_torch(B) else np.array(B, dtype=np.complex128, order="C")
        return self.ldiv_batch_(V)

    def batch_info(self):
        """lsfc_precond_batch_info as a dict (BATCH_FIELDS): group sweeps enqueued, vectors that went through them, the
        largest group and the bytes of group work buffers; all 0 on an object of the host-LU route"""
        out = (C.c_int64 * len(BATCH_FIELDS))()
        L.check(L.load().lsfc_precond_batch_info(self._pc, out))
        return dict(zip(BATCH_FIELDS, (int(v) for v in out)))

    def set_stream(self, stream):
        L.check(L.load().lsfc_precond_set_stream(self._pc, C.c_void_p(int(stream))))

    def stats(self):
        """dependency levels of the L and U solves, kernel launches captured in the graph, and what the launch schedule
        of each solve reached (schedule_L / schedule_U, SCHEDULE_FIELDS of lsfc_precond_schedule).  A block-tridiagonal
        object has no levels: levels_L = levels_U = its blocks, and the fields of `blocktri_info` take the schedule's place."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        lib = L.load()
        L.check(lib.lsfc_precond_stats(self._pc, C.byref(a), C.byref(b), C.byref(c)))
        if self.factor == "blocktri":
            return {"levels_L": a.value, "levels_U": b.value, **self.blocktri_info(), "launches": c.value}
        st = {"levels_L": a.value, "levels_U": b.value, "launches": c.value, "nnz_L": self.nnz_L, "nnz_U": self.nnz_U}
        for factor, name in ((0, "schedule_L"), (1, "schedule_U")):
            out = (C.c_int64 * len(SCHEDULE_FIELDS))()
            L.check(lib.lsfc_precond_schedule(self._pc, factor, out))
            st[name] = dict(zip(SCHEDULE_FIELDS, out))
        return st

    def close(self):
        if getattr(self, "_pc", None):
            L.load().lsfc_precond_destroy(self._pc)
            self._pc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def _op_of(P):
    """The object behind P means P.T or P.H while a call through such a view runs, and P again afterwards (also when it
    raises).  The first use of a view builds the transposed tables on the device (not inside a stream capture)."""
    op = getattr(P, "_op", L.LSFC_OP_N)
    if op == L.LSFC_OP_N:
        yield
        return
    lib = L.load()
    L.check(lib.lsfc_precond_set_op(P._pc, op))
    try:
        yield
    finally:
        lib.lsfc_precond_set_op(P._pc, L.LSFC_OP_N)


class PreconditionerView:
    """P.T or P.H: the parent preconditioner plus an op, no second object and no second copy of the inverses.  Accepted as
    ``Pl`` of the four solvers with the operator view of the same op (M.T with P.T, M.H with P.H).  A call through a view
    sets the op of the parent's object, calls, and restores P.  conj(P) is not offered, so P.T.H and P.H.T raise.  Only a
    block-tridiagonal parent has views: the host-LU route has no transposed solves."""

    def __init__(self, parent, op):
        if getattr(parent, "factor", None) != "blocktri":
            raise ValueError("P.T / P.H need a block-tridiagonal preconditioner (factor='blocktri' or from_operator): the host-LU "
                             "route has no transposed triangular solves")
        self.parent, self._op = parent, op

    @property
    def _pc(self):
        return self.parent._pc

    @property
    def N(self):
        return self.parent.N

    def _other(self, op, name):
        if op == self._op:
            return self.parent
        raise NotImplementedError(f"{name}: conj(P) is not offered (only P, P.T and P.H)")

    def transpose(self):
        return self._other(L.LSFC_OP_T, "P.H.T")

    def adjoint(self):
        return self._other(L.LSFC_OP_H, "P.T.H")

    T = property(transpose)
    H = property(adjoint)

    def ldiv_(self, v):
        with _op_of(self):
            return self.parent.ldiv_(v)

    def __call__(self, v):
        self.ldiv_(v)

    def solve(self, b):
        with _op_of(self):
            return self.parent.solve(b)

    def ldiv_batch_(self, V):
        with _op_of(self):
            return self.parent.ldiv_batch_(V)

    def solve_batch(self, B):
        with _op_of(self):
            return self.parent.solve_batch(B)

    def set_stream(self, stream):
        self.parent.set_stream(stream)
