"""CPU tests of the transposed / adjoint operator's boundary: the three entry points and the constants exist in the header, the
library and the binding; argument errors come back as LSFC_EINVAL before any device call; the views M.T / M.H compose as
documented.  No compute is attempted here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lsfc_plan_set_op", "lsfc_plan_get_op", "lsfc_plan_symmetry_defect")


def test_entry_points_and_constants_are_declared_exported_and_bound():
    import fast_solver_lippmann_schwinger_amd._lib as L
    text = open(os.path.join(ROOT, "include", "lsfc.h")).read()
    for name, value in (("LSFC_OP_N", 0), ("LSFC_OP_T", 1), ("LSFC_OP_H", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(L, name) == value
    lib = C.CDLL(L.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in L.SIGNATURES, f"{name} not bound"
    assert L.SIGNATURES["lsfc_plan_set_op"][1] == [C.c_void_p, C.c_int]
    # the header says what the op does not touch, and what is out of scope
    for word in ("lsfc_convolve", "lsfc_sample_sources", "lsfc_sparsify_build", "lsfc_precond_create_from_plan", "Out of scope"):
        assert word in text[text.index("the transposed and the adjoint operator"):text.index("#define LSFC_OP_N")], word


def test_null_plan_and_bad_op_are_einval_without_a_device():
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    op, d = C.c_int(-7), C.c_double(-7.0)
    for bad in (-1, 3, 17):
        assert lib.lsfc_plan_set_op(None, bad) == L.LSFC_EINVAL
        assert "op must be" in lib.lsfc_last_error().decode()
    for good in (L.LSFC_OP_N, L.LSFC_OP_T, L.LSFC_OP_H):
        assert lib.lsfc_plan_set_op(None, good) == L.LSFC_EINVAL
        assert "NULL" in lib.lsfc_last_error().decode()
    assert lib.lsfc_plan_get_op(None, C.byref(op)) == L.LSFC_EINVAL and op.value == -7
    assert lib.lsfc_plan_symmetry_defect(None, C.byref(d)) == L.LSFC_EINVAL and d.value == -7.0
    with pytest.raises(L.LsfcError) as ei:
        L.check(lib.lsfc_plan_set_op(None, 1))
    assert ei.value.code == L.LSFC_EINVAL


def _planless_operator():
    """an operator object without a plan (none can be made without a device): enough for the algebra of the views"""
    import fast_solver_lippmann_schwinger_amd as pkg
    M = object.__new__(pkg.FastM3D)
    M.nu = np.zeros(24)
    return pkg, M


def test_view_algebra():
    import fast_solver_lippmann_schwinger_amd._lib as L
    pkg, M = _planless_operator()
    T, H = M.T, M.H
    assert isinstance(T, pkg.OperatorView) and isinstance(H, pkg.OperatorView)
    assert T._op == L.LSFC_OP_T and H._op == L.LSFC_OP_H and T.parent is M and H.parent is M
    assert M.transpose()._op == L.LSFC_OP_T and M.adjoint()._op == L.LSFC_OP_H
    assert T.T is M and H.H is M and T.transpose() is M and H.adjoint() is M
    for f in (lambda: T.H, lambda: H.T, T.adjoint, H.transpose):
        with pytest.raises(NotImplementedError):
            f()
    # light: the parent's plan and traits, no second plan
    assert T._plan is M._plan and T.shape == (24, 24) == H.shape and T.dtype == np.complex128 and T.size(1) == 24
    assert T.size() == M.size() and T.eltype() == np.complex128
    for name in ("N", "size", "shape", "dtype", "matvec", "mul_", "_plan", "__mul__", "__matmul__"):
        assert hasattr(pkg.OperatorView, name), name
    for name in ("T", "H", "transpose", "adjoint", "rmatvec", "aslinearoperator", "symmetry_defect"):
        assert hasattr(pkg.FastM, name) and hasattr(pkg.FastM3D, name), name
