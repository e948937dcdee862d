"""CPU tests of the single-precision storage of the preconditioner's Schur inverses (LSFC_PRECOND_INV_F32): the header,
the ctypes binding and the library declare the three new entry points, the argument errors of the C ABI and of the
Python class are raised without a device, and the numerical premise is pinned on the numpy restatement
(tests/blocktri_ref.py): rounding every S_k^{-1} of `eliminate` to complex64 moves `solve` by less than 1e-6 relative,
and no stored part is near the float denormal range."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import blocktri_ref as bt
from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lsfc_precond_create_blocktri_prec": 10, "lsfc_precond_create_from_plan_prec": 3, "lsfc_precond_inverse_precision": 2}
LSFC_EINVAL = -1
FLOAT_MIN_NORMAL = float(np.finfo(np.float32).tiny)        # 1.18e-38


def _header():
    text = open(os.path.join(ROOT, "include", "lsfc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_binding_and_library_declare_the_new_entries():
    import fast_solver_lippmann_schwinger_amd._lib as L
    protos = dict(re.findall(r"\b(lsfc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S))
    lib = C.CDLL(L.LIB_PATH)
    for name, nparams in NEW.items():
        assert name in protos, f"{name} is not declared in include/lsfc.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
        assert len([a for a in protos[name].split(",") if a.strip()]) == nparams == len(L.SIGNATURES[name][1])
    assert re.search(r"#define\s+LSFC_PRECOND_INV_F64\s+0\b", _header()) and re.search(r"#define\s+LSFC_PRECOND_INV_F32\s+1\b", _header())
    assert (L.LSFC_PRECOND_INV_F64, L.LSFC_PRECOND_INV_F32) == (0, 1)
    # the last parameter of both constructors is the precision, an int
    for name in ("lsfc_precond_create_blocktri_prec", "lsfc_precond_create_from_plan_prec"):
        assert re.search(r"int\s+inverse_precision\s*$", protos[name].strip()), name
        assert L.SIGNATURES[name][1][-1] is C.c_int
    assert L.SIGNATURES["lsfc_precond_inverse_precision"][1][1] is C.POINTER(C.c_int)


def test_a_bad_precision_is_refused_before_any_device_call():
    # this machine may have no device: LSFC_EINVAL (not LSFC_ENODEV) shows that the value was looked at first
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    rowptr = np.arange(3, dtype=np.int64)
    col = np.arange(2, dtype=np.int64)
    val = np.ones(2, dtype=np.complex128)
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    stand_in = (C.c_char * 4096)()                         # a non-NULL plan address that is never read
    for bad in (-1, 2, 64):
        pc = C.c_void_p()
        assert lib.lsfc_precond_create_blocktri_prec(C.byref(pc), 2, 2, p(rowptr), p(col), p(val), p(val), L.LSFC_MEM_HOST, 0, bad) == LSFC_EINVAL
        assert "inverse_precision" in lib.lsfc_last_error().decode() and not pc.value
        assert lib.lsfc_precond_create_from_plan_prec(C.byref(pc), C.cast(stand_in, C.c_void_p), bad) == LSFC_EINVAL
        assert "inverse_precision" in lib.lsfc_last_error().decode() and not pc.value
    assert bytes(stand_in) == bytes(4096)
    prec = C.c_int(7)
    assert lib.lsfc_precond_inverse_precision(None, C.byref(prec)) == LSFC_EINVAL and prec.value == 7


def test_python_argument_errors_without_a_device():
    import scipy.sparse as sp
    from fast_solver_lippmann_schwinger_amd.preconditioner import SparsifyingPreconditioner, INVERSE_DTYPES
    assert INVERSE_DTYPES == {"complex128": 0, "complex64": 1}
    assert isinstance(SparsifyingPreconditioner.inverse_dtype, property)
    eye = sp.identity(4, dtype=np.complex128, format="csr")
    for bad in ("float32", "complex32", np.complex64, None, 1):
        with pytest.raises(ValueError, match="inverse_dtype"):
            SparsifyingPreconditioner(eye, eye, factor="blocktri", nblocks=2, inverse_dtype=bad)
        with pytest.raises(ValueError, match="inverse_dtype"):
            SparsifyingPreconditioner.from_operator(object(), inverse_dtype=bad)
    with pytest.raises(ValueError, match="blocktri"):
        SparsifyingPreconditioner(eye, eye, factor="host", inverse_dtype="complex64")
    with pytest.raises(ValueError, match="blocktri"):
        SparsifyingPreconditioner(eye, eye, inverse_dtype="complex64")


@pytest.mark.parametrize("kind,dims", [("trap", (33, 33)), ("gv3d", (12, 12, 12))])
def test_rounding_the_inverses_to_complex64_moves_the_solve_by_less_than_1e_6(kind, dims):
    Msp, As = bt.ref_pair(kind, dims)
    K = dims[-1]
    Sinv = bt.eliminate(Msp, K)
    parts = np.concatenate([np.abs(np.concatenate([S.real.ravel(), S.imag.ravel()])) for S in Sinv])
    smallest = parts[parts > 0].min()
    rounded = [S.astype(np.complex64).astype(np.complex128) for S in Sinv]
    rng = np.random.default_rng(3)
    v = rng.standard_normal(Msp.shape[0]) + 1j * rng.standard_normal(Msp.shape[0])
    w = As @ v
    change = rel_err(bt.solve(Msp, rounded, w), bt.solve(Msp, Sinv, w))
    print(f"{kind} {dims}: relative l2 change of Msp^-1 (As v) {change:.2e}, smallest nonzero part of any S_k^-1 {smallest:.2e}")
    assert smallest >= FLOAT_MIN_NORMAL
    assert 0.0 < change < 1e-6
