"""CPU tests of the complex-nu boundary: the two entry points exist in the header, the library and the binding with the right
prototypes; NULL arguments come back as LSFC_EINVAL before any device call; the header no longer lists complex nu as out of
scope and states the conjugation rule; the Python front end keeps the dtype rule.  No compute is attempted here."""
import ctypes as C
import os
import re
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lsfc_plan_set_nu_complex", "lsfc_plan_nu_is_complex")


def _header():
    return open(os.path.join(ROOT, "include", "lsfc.h")).read()


def test_entry_points_are_declared_exported_and_bound():
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = C.CDLL(L.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in L.SIGNATURES, f"{name} not bound"
    assert re.search(r"int\s+lsfc_plan_set_nu_complex\s*\(\s*lsfc_plan\s*\*\s*plan\s*,\s*const\s+double\s*\*\s*nu\s*,\s*int\s+memspace\s*\)", code)
    assert re.search(r"int\s+lsfc_plan_nu_is_complex\s*\(\s*const\s+lsfc_plan\s*\*\s*plan\s*,\s*int\s*\*\s*is_complex\s*\)", code)
    assert L.SIGNATURES["lsfc_plan_set_nu_complex"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int])
    assert L.SIGNATURES["lsfc_plan_set_nu_complex"] == L.SIGNATURES["lsfc_plan_set_nu"]
    assert L.SIGNATURES["lsfc_plan_nu_is_complex"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])


def test_null_arguments_are_einval_without_a_device():
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    nu = np.zeros(8)
    flag = C.c_int(-7)
    for memspace in (L.LSFC_MEM_HOST, L.LSFC_MEM_DEVICE):
        assert lib.lsfc_plan_set_nu_complex(None, nu.ctypes.data_as(C.c_void_p), memspace) == L.LSFC_EINVAL
        assert "NULL" in lib.lsfc_last_error().decode()
        assert lib.lsfc_plan_set_nu_complex(None, None, memspace) == L.LSFC_EINVAL
    assert lib.lsfc_plan_nu_is_complex(None, C.byref(flag)) == L.LSFC_EINVAL and flag.value == -7
    assert "NULL" in lib.lsfc_last_error().decode()


def test_header_has_complex_nu_in_scope_and_states_the_rule():
    text = _header()
    op = text[text.index("the transposed and the adjoint operator"):text.index("#define LSFC_OP_N")]
    scope = op[op.index("Out of scope"):]
    assert "complex nu" not in scope and "complex" not in scope.lower()
    assert "nu and omega are real" not in text
    assert "conjugation is outermost" in op.lower() and "conj(nu)" in op
    doc = text[text.index("lsfc_plan_set_nu(lsfc_plan* plan"):text.index("int lsfc_plan_nu_is_complex")]
    for word in ("interleaved", "lsfc_apply_batch", "lsfc_sparsify_build", "lsfc_precond_create_from_plan", "distributed", "multi-device"):
        assert word in doc, word


def test_python_dtype_rule_without_a_device():
    """a real dtype stays float64, a complex dtype stays complex128 even with zero imaginary part, and nothing is dropped"""
    import fast_solver_lippmann_schwinger_amd as pkg
    import fast_solver_lippmann_schwinger_amd.operators as ops
    with warnings.catch_warnings():
        warnings.simplefilter("error")                           # (a dropped imaginary part raises numpy's ComplexWarning)
        c = ops._nu_array(np.array([[1 + 2j, 3 - 1j]]))
        z = ops._nu_array(np.array([1.0, 2.0], dtype=np.complex64))
        r = ops._nu_array([1, 2, 3])
    assert c.dtype == np.complex128 and c.shape == (2,) and c[1] == 3 - 1j
    assert z.dtype == np.complex128 and np.all(z.imag == 0)
    assert r.dtype == np.float64
    assert ops._nu_real_part(c).dtype == np.float64 and ops._nu_real_part(c).flags.c_contiguous and ops._nu_real_part(r) is r
    # an operator object around an existing plan keeps the dtype it was given
    M = pkg.FastM3D(None, c, 8, 4, 4, 2, 1, 1, 1.0, _plan=C.c_void_p())
    assert M.nu.dtype == np.complex128 and M.shape == (2, 2)
    M._plan = None
    for cls in (pkg.FastM, pkg.FastM3D):
        assert isinstance(cls.nu_is_complex, property)
    assert "nu and omega are real" not in (pkg.FastM.adjoint.__doc__ or "")
