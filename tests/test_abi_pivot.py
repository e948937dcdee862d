"""The ABI of partial pivoting in the block-tridiagonal preconditioner: the three entry points and the three constants
exist in the built library, in include/lsfc.h and in _lib.py, and lsfc_blocktri_opts is eight ints.  No GPU."""
import ctypes as C
import os
import re

import fast_solver_lippmann_schwinger_amd._lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsfc.h")
SYMBOLS = ("lsfc_precond_create_blocktri_opts", "lsfc_precond_create_from_plan_opts", "lsfc_precond_blocktri_get_pivots")
CONSTANTS = {"LSFC_PRECOND_PIVOT_NONE": 0, "LSFC_PRECOND_PIVOT_PARTIAL": 1, "LSFC_PRECOND_PIVOT_AUTO": 2}


def test_symbols_in_the_library_and_the_binding():
    lib = L.load()
    for name in SYMBOLS:
        fn = getattr(lib, name)                            # AttributeError if the library does not export it
        assert fn.restype is C.c_int and fn.argtypes is not None, name
    assert len(lib.lsfc_precond_create_blocktri_opts.argtypes) == 10
    assert len(lib.lsfc_precond_create_from_plan_opts.argtypes) == 3
    assert len(lib.lsfc_precond_blocktri_get_pivots.argtypes) == 4


def test_constants_and_struct():
    text = open(HEADER).read()
    for name, value in CONSTANTS.items():
        assert getattr(L, name) == value
        m = re.search(rf"#define\s+{name}\s+(\d+)", text)
        assert m and int(m.group(1)) == value, name
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    assert re.search(r"typedef struct lsfc_blocktri_opts \{ int inverse_precision; int pivoting; int reserved\[6\]; \} lsfc_blocktri_opts;", text)
    assert C.sizeof(L.BlocktriOpts) == 8 * C.sizeof(C.c_int)
    assert [f[0] for f in L.BlocktriOpts._fields_] == ["inverse_precision", "pivoting", "reserved"]
    o = L.BlocktriOpts(inverse_precision=1, pivoting=2)
    assert list(o.reserved) == [0] * 6 and C.cast(C.byref(o), C.POINTER(C.c_int))[1] == 2


def test_python_keyword_is_checked_without_a_device():
    import numpy as np
    import pytest
    import scipy.sparse as sp
    import fast_solver_lippmann_schwinger_amd as lsfc
    eye = sp.identity(4, dtype=np.complex128, format="csr")
    with pytest.raises(ValueError, match="pivoting"):
        lsfc.SparsifyingPreconditioner(eye, eye, factor="blocktri", nblocks=2, pivoting="full")
    with pytest.raises(ValueError, match="blocktri"):
        lsfc.SparsifyingPreconditioner(eye, eye, pivoting="auto")
