"""ctypes binding of liblsfc.so (include/lsfc.h).  There is no Python or CPU
fallback: if the HIP library is missing the import of the compute path fails
loudly, and every compute entry point returns LSFC_ENODEV without a GPU."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (developer override for A/B builds: LSFC_LIBRARY=/path/to/another/liblsfc.so; a missing file is an error either way)
LIB_PATH = os.environ.get("LSFC_LIBRARY") or os.path.join(_HERE, "liblsfc.so")

LSFC_QUAD_TRAPEZOIDAL, LSFC_QUAD_GREENGARD_VICO = 0, 1
LSFC_MEM_HOST, LSFC_MEM_DEVICE = 0, 1
LSFC_PRECOND_INV_F64, LSFC_PRECOND_INV_F32 = 0, 1
LSFC_PRECOND_PIVOT_NONE, LSFC_PRECOND_PIVOT_PARTIAL, LSFC_PRECOND_PIVOT_AUTO = 0, 1, 2
LSFC_FLAG_DEFAULT, LSFC_FLAG_LITERAL_PAD, LSFC_FLAG_FORCE_ROCFFT, LSFC_FLAG_PATCH_SINGULAR = 0, 1, 2, 4
LSFC_ORTH_MGS, LSFC_ORTH_CGS, LSFC_ORTH_DGKS = 0, 1, 2
LSFC_EINVAL, LSFC_ENODEV, LSFC_ENOMEM, LSFC_ENOTCONV = -1, -2, -3, -5
LSFC_UNIQUE_ID_BYTES = 128
LSFC_OP_N, LSFC_OP_T, LSFC_OP_H = 0, 1, 2
LSFC_RECV_POINTS, LSFC_RECV_FARFIELD = 0, 1
LSFC_BORN_ACCUMULATE, LSFC_BORN_REAL = 1, 2
LSFC_BORN_GMRES, LSFC_BORN_BICGSTABL = 0, 1
LSFC_BORN_ADJOINT_STATE, LSFC_BORN_RECIPROCAL = 0, 1
# how a member of lsfc_bicgstabl_batch ended (status[2 j]); 2..7: the scalar of a breakdown
(LSFC_BICG_CONVERGED, LSFC_BICG_MAX_MV, LSFC_BICG_RHO, LSFC_BICG_SIGMA, LSFC_BICG_BETA, LSFC_BICG_ALPHA, LSFC_BICG_GAMMA,
 LSFC_BICG_RESIDUAL) = range(8)

PRECOND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)


class GmresOpts(C.Structure):
    _fields_ = [("restart", C.c_int), ("maxiter", C.c_int64), ("reltol", C.c_double), ("abstol", C.c_double),
                ("orth", C.c_int), ("initially_zero", C.c_int), ("precond", PRECOND_FN), ("precond_user", C.c_void_p),
                ("precond_on_device", C.c_int)]


class GmresResult(C.Structure):
    _fields_ = [("iters", C.c_int64), ("mvps", C.c_int64), ("converged", C.c_int), ("final_resnorm", C.c_double)]


class BicgstablOpts(C.Structure):                  # lsfc_bicgstabl_opts
    _fields_ = [("l", C.c_int), ("max_mv_products", C.c_int64), ("reltol", C.c_double), ("abstol", C.c_double),
                ("initially_zero", C.c_int), ("precond", PRECOND_FN), ("precond_user", C.c_void_p),
                ("precond_on_device", C.c_int), ("r_shadow", C.c_void_p), ("reserved", C.c_int * 4)]


class BlocktriOpts(C.Structure):                   # lsfc_blocktri_opts
    _fields_ = [("inverse_precision", C.c_int), ("pivoting", C.c_int), ("reserved", C.c_int * 6)]


class BornOpts(C.Structure):                       # lsfc_born_opts
    _fields_ = [("solver", C.c_int), ("restart", C.c_int), ("l", C.c_int), ("maxiter", C.c_int64), ("reltol", C.c_double),
                ("abstol", C.c_double), ("precond", C.c_void_p), ("chunk", C.c_int64), ("reserved", C.c_int * 6)]


class LsfcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lsfc error {code}: {msg}")
        self.code = code


# every symbol include/lsfc.h declares: name -> (restype, argtypes)
_P, _I, _L, _D, _U = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_uint
_PP = C.POINTER(C.c_void_p)
SIGNATURES = {
    "lsfc_plan_create_2d": (_I, [_PP, _L, _L, _L, _L, _P, _P, _D, _I, _U, _I]),
    "lsfc_plan_create_3d": (_I, [_PP, _L, _L, _L, _L, _L, _L, _P, _P, _D, _I, _U, _I]),
    "lsfc_plan_create_gv2d": (_I, [_PP, _L, _L, _D, _D, _P, _U, _I]),
    "lsfc_plan_create_trap2d": (_I, [_PP, _L, _L, _D, _D, _D, _D, _D, _D, _P, _U, _I]),
    "lsfc_plan_create_gv3d": (_I, [_PP, _L, _L, _L, _D, _D, _P, _U, _I]),
    "lsfc_plan_destroy": (_I, [_P]),
    "lsfc_plan_size": (_L, [_P]),
    "lsfc_plan_dims": (_I, [_P, C.POINTER(_L), C.POINTER(_L)]),
    "lsfc_plan_pipeline": (C.c_char_p, [_P]),
    "lsfc_plan_set_nu": (_I, [_P, _P, _I]),
    "lsfc_plan_set_nu_complex": (_I, [_P, _P, _I]),
    "lsfc_plan_nu_is_complex": (_I, [_P, C.POINTER(C.c_int)]),
    "lsfc_plan_get_symbol": (_I, [_P, _P, _L, C.POINTER(_L)]),
    "lsfc_plan_set_op": (_I, [_P, _I]),
    "lsfc_plan_get_op": (_I, [_P, C.POINTER(_I)]),
    "lsfc_plan_symmetry_defect": (_I, [_P, C.POINTER(_D)]),
    "lsfc_apply": (_I, [_P, _P, _P, _I]),
    "lsfc_convolve": (_I, [_P, _P, _P, _I, _I]),
    "lsfc_apply_batch": (_I, [_P, _P, _P, _L, _I, _I]),
    "lsfc_sample_sources": (_I, [_P, _P, _L, _P, _I]),
    "lsfc_gmres": (_I, [_P, _P, _P, C.POINTER(GmresOpts), _P, _L, C.POINTER(GmresResult), _I]),
    "lsfc_gmres_batch": (_I, [_P, _P, _P, _L, C.POINTER(GmresOpts), _P, _L, C.POINTER(GmresResult), _I]),
    "lsfc_bicgstabl": (_I, [_P, _P, _P, C.POINTER(BicgstablOpts), _P, _L, C.POINTER(GmresResult), _I]),
    "lsfc_bicgstabl_multi": (_I, [_P, _P, _P, C.POINTER(BicgstablOpts), _P, _L, C.POINTER(GmresResult), _I]),
    "lsfc_bicgstabl_batch": (_I, [_P, _P, _P, _L, C.POINTER(BicgstablOpts), _P, _L, C.POINTER(GmresResult), _P, _I]),
    "lsfc_precond_create": (_I, [_PP, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "lsfc_precond_destroy": (_I, [_P]),
    "lsfc_precond_set_stream": (_I, [_P, _P]),
    "lsfc_precond_set_op": (_I, [_P, _I]),
    "lsfc_precond_get_op": (_I, [_P, C.POINTER(_I), C.POINTER(_L)]),
    "lsfc_precond_apply": (_I, [_P, _P, _I]),
    "lsfc_precond_apply_batch": (_I, [_P, _P, _L, _I]),
    "lsfc_precond_batch_info": (_I, [_P, C.POINTER(_L)]),
    "lsfc_precond_callback": (_I, [_P, _P, _L]),
    "lsfc_precond_stats": (_I, [_P, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L)]),
    "lsfc_precond_schedule": (_I, [_P, _I, C.POINTER(_L)]),
    "lsfc_precond_create_blocktri": (_I, [_PP, _L, _L, _P, _P, _P, _P, _I, _I]),
    "lsfc_precond_create_from_plan": (_I, [_PP, _P]),
    "lsfc_precond_create_blocktri_prec": (_I, [_PP, _L, _L, _P, _P, _P, _P, _I, _I, _I]),
    "lsfc_precond_create_from_plan_prec": (_I, [_PP, _P, _I]),
    "lsfc_precond_create_blocktri_opts": (_I, [_PP, _L, _L, _P, _P, _P, _P, _I, _I, _P]),
    "lsfc_precond_create_from_plan_opts": (_I, [_PP, _P, _P]),
    "lsfc_precond_blocktri_get_pivots": (_I, [_P, _L, _P, _L]),
    "lsfc_precond_inverse_precision": (_I, [_P, C.POINTER(_I)]),
    "lsfc_precond_blocktri_info": (_I, [_P, C.POINTER(_L), C.POINTER(_D)]),
    "lsfc_precond_blocktri_get_block": (_I, [_P, _L, _P, _L]),
    "lsfc_receivers_create": (_I, [_PP, _I, C.POINTER(_L), C.POINTER(_D), _D, _D, _I, _P, _L, _I]),
    "lsfc_receivers_destroy": (_I, [_P]),
    "lsfc_receivers_set_stream": (_I, [_P, _P]),
    "lsfc_receivers_apply": (_I, [_P, _P, _P, _P, _L, _I, _I]),
    "lsfc_receivers_info": (_I, [_P, C.POINTER(_L)]),
    "lsfc_born_scale": (_I, [_P, _P, _I, _P, _P, _L, _I]),
    "lsfc_born_image": (_I, [_P, _P, _P, _L, _D, _D, _U, _P, _I]),
    "lsfc_born_create": (_I, [_PP, _P, _P, C.POINTER(BornOpts)]),
    "lsfc_born_destroy": (_I, [_P]),
    "lsfc_born_set_background": (_I, [_P, _P, _L, _I]),
    "lsfc_born_fields": (_I, [_P, _PP, C.POINTER(_L)]),
    "lsfc_born_data": (_I, [_P, _P, _I]),
    "lsfc_born_apply": (_I, [_P, _P, _I, _P, _I, _U, _I]),
    "lsfc_born_info": (_I, [_P, C.POINTER(_L), C.POINTER(GmresResult)]),
    "lsfc_born_contract": (_I, [_P, _P, _L, _P, _L, _P, _I, _P, _I, _U, _D, _D, _I]),
    "lsfc_born_set_mode": (_I, [_P, _I]),
    "lsfc_born_get_mode": (_I, [_P, C.POINTER(_I), C.POINTER(_L)]),
    "lsfc_born_receiver_fields": (_I, [_P, _PP, C.POINTER(_L)]),
    "lsfc_born_receiver_info": (_I, [_P, C.POINTER(_L), C.POINTER(GmresResult)]),
    "lsfc_sparsify_pattern": (_I, [_L, _L, _L, C.POINTER(_L), _P, _P, _P]),
    "lsfc_sparsify_build": (_I, [_P, _P, _P, _P, _P, _P, _P, _I]),
    "lsfc_plan_set_stream": (_I, [_P, _P]),
    "lsfc_plan_synchronize": (_I, [_P]),
    "lsfc_plan_set_tuning": (_I, [_P, C.c_char_p, _I]),
    "lsfc_plan_describe_passes": (_I, [_P, _I, C.c_char_p, _L, C.POINTER(_L)]),
    "lsfc_time_apply": (_I, [_P, _P, _P, _I, C.POINTER(_D)]),
    "lsfc_profile_apply": (_I, [_P, _P, _P, _I, _I, C.POINTER(C.c_char_p), C.POINTER(_D), C.POINTER(_D), C.POINTER(_I)]),
    "lsfc_device_count": (_I, [C.POINTER(_I)]),
    "lsfc_malloc": (_I, [_PP, C.c_size_t, _I]),
    "lsfc_free": (_I, [_P]),
    "lsfc_memcpy_h2d": (_I, [_P, _P, C.c_size_t]),
    "lsfc_memcpy_d2h": (_I, [_P, _P, C.c_size_t]),
    "lsfc_host_register": (_I, [_P, C.c_size_t]),
    "lsfc_host_unregister": (_I, [_P]),
    "lsfc_host_alloc": (_I, [_PP, C.c_size_t]),
    "lsfc_host_free": (_I, [_P]),
    "lsfc_dist_unique_id": (_I, [_P]),
    "lsfc_dist_plan_create_gv3d": (_I, [_PP, _L, _L, _L, _D, _D, _P, _U, _I, _I, _I, _P]),
    "lsfc_dist_sim_plan_create_gv3d": (_I, [_PP, _L, _L, _L, _D, _D, _P, _U, _I, _I, _I]),
    "lsfc_dist_sim_apply": (_I, [_PP, _I, _PP, _PP, _I]),
    "lsfc_plan_create_gv3d_multi": (_I, [_PP, _L, _L, _L, _D, _D, _P, _U, C.POINTER(_I), _I]),
    "lsfc_multi_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_L), C.POINTER(C.c_char_p)]),
    "lsfc_multi_apply_dev": (_I, [_P, _PP, _PP, _I]),
    "lsfc_last_error": (C.c_char_p, []),
    "lsfc_padded_length": (_I, [C.c_int64]),
    "lsfc_storage_order": (_I, [_L, C.POINTER(_L)]),
    "lsfc_version": (C.c_char_p, []),
}

_lib = None


def load():
    """Load liblsfc.so (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback for the lsfc operator")
        try:
            # PyTorch-ROCm bundles its own HIP runtime; when both live in one process torch's copy must be
            # loaded first, otherwise torch.cuda later reports "No HIP GPUs are available".
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise LsfcError(rc, load().lsfc_last_error().decode(errors="replace"))
    return rc


def host_register(a):
    """Page-lock a long-lived numpy vector (lsfc_host_register): host-vector applies then move it by DMA."""
    check(load().lsfc_host_register(a.ctypes.data_as(C.c_void_p), a.nbytes))


def host_unregister(a):
    check(load().lsfc_host_unregister(a.ctypes.data_as(C.c_void_p)))


class _PinnedBlock:
    """owner of one lsfc_host_alloc block; freed when the last numpy view of it is gone"""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        check(load().lsfc_host_alloc(C.byref(self.ptr), max(int(nbytes), 1)))
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                load().lsfc_host_free(self.ptr)
                self.ptr = C.c_void_p()
        except Exception:
            pass


def host_empty(shape, dtype="complex128"):
    """numpy array in page-locked memory owned by the HIP runtime (lsfc_host_alloc): host-vector applies move it by DMA.
    The preferred form of a page-locked work vector (page-aligned, shares no page with the process heap)."""
    import numpy as np
    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    blk = _PinnedBlock(count * dt.itemsize)
    buf = (C.c_char * max(blk.nbytes, 1)).from_address(blk.ptr.value)
    buf._owner = blk                               # numpy keeps `buf` (its base) alive, `buf` keeps the block alive
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def device_count():
    n = C.c_int(0)
    load().lsfc_device_count(C.byref(n))
    return n.value
