"""The ABI of lsfc_bicgstabl_batch: the entry point exists in the built library, in include/lsfc.h and in _lib.py, the public
LSFC_BICG_* codes agree between header and binding, and the argument checks that come before any device call answer
without a GPU."""
import ctypes as C
import os
import re

import numpy as np

import fast_solver_lippmann_schwinger_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsfc.h")
CODES = ["CONVERGED", "MAX_MV", "RHO", "SIGMA", "BETA", "ALPHA", "GAMMA", "RESIDUAL"]


def test_symbol_in_the_library_and_the_binding():
    fn = L.load().lsfc_bicgstabl_batch
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+lsfc_bicgstabl_batch\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
    params = [p.strip() for p in proto.split(",")]
    assert len(params) == 10 and "lsfc_bicgstabl_opts" in proto and "lsfc_gmres_result" in proto
    assert params[3] == "int64_t nrhs" and params[8] == "int64_t* status" and params[9] == "int memspace"
    import fast_solver_lippmann_schwinger_amd as pkg
    assert callable(pkg.bicgstabl_batch_) and "bicgstabl_batch_" in pkg.__all__
    # the single solve no longer lists the batch form as missing
    assert "a lock-step batch form" not in open(HEADER).read()
    assert "function bicgstabl_batch_hip!" in open(os.path.join(ROOT, "julia", "FastConvHIP.jl")).read()


def test_codes_agree_between_header_and_binding():
    text = open(HEADER).read()
    for value, name in enumerate(CODES):
        m = re.search(rf"#define\s+LSFC_BICG_{name}\s+(\d+)", text)
        assert m, name
        assert int(m.group(1)) == value == getattr(L, f"LSFC_BICG_{name}"), name
    # codes 2..7 in the order of the solver's status words ST_RHO ... ST_RESIDUAL
    src = open(os.path.join(ROOT, "fast_solver_lippmann_schwinger_amd", "csrc", "bicgstab.hip")).read()
    st = re.search(r"enum \{ ST_OK = 0, ST_EXHAUSTED = 1, (.*?) \};", src).group(1)
    assert [s.split("=")[0].strip() for s in st.split(",")] == [f"ST_{n}" for n in CODES[2:]]
    assert [int(s.split("=")[1]) for s in st.split(",")] == list(range(2, 8))


def test_argument_checks_before_any_device_call():
    # (no plan can exist without a GPU: the checks on nrhs, opts and memspace come first and do not look at the plan)
    lib = L.load()
    X, B = np.zeros((2, 4), complex), np.ones((2, 4), complex)
    px, pb = X.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p)
    res = (L.GmresResult * 2)()
    status = np.full(4, -7, dtype=np.int64)
    ok = C.byref(L.BicgstablOpts(l=2))

    def call(opts, nrhs=2, plan=None, memspace=L.LSFC_MEM_HOST, results=res):
        rc = lib.lsfc_bicgstabl_batch(plan, px, pb, nrhs, opts, None, 0, results, status.ctypes.data_as(C.c_void_p), memspace)
        return rc, lib.lsfc_last_error().decode()

    rc, msg = call(None)
    assert rc == L.LSFC_EINVAL and "NULL opts" in msg
    for l in (0, 9, -1):
        rc, msg = call(C.byref(L.BicgstablOpts(l=l)))
        assert rc == L.LSFC_EINVAL and "1..8" in msg and str(l) in msg
    for i in range(4):
        o = L.BicgstablOpts(l=2)
        o.reserved[i] = 1
        rc, msg = call(C.byref(o))
        assert rc == L.LSFC_EINVAL and f"reserved[{i}]" in msg
    rc, msg = call(ok, memspace=2)
    assert rc == L.LSFC_EINVAL and "memspace" in msg
    for nrhs in (0, 65, -1):
        rc, msg = call(ok, nrhs=nrhs)
        assert rc == L.LSFC_EINVAL and "1..64" in msg and str(nrhs) in msg
    rc, msg = call(ok)                                                  # NULL plan
    assert rc == L.LSFC_EINVAL and "NULL argument" in msg
    rc, msg = call(ok, plan=C.c_void_p(8), results=None)                # NULL results: refused before the plan is read
    assert rc == L.LSFC_EINVAL and "NULL argument" in msg
    assert np.all(X == 0) and np.all(status == -7)


def test_wrapper_refuses_bad_arrays_before_the_library():
    import fast_solver_lippmann_schwinger_amd as pkg
    import pytest
    import types
    A = types.SimpleNamespace(N=4, _plan=None)
    X = np.zeros((2, 4), complex)
    with pytest.raises(ValueError):
        pkg.bicgstabl_batch_(X, A, np.ones((3, 4), complex))
    with pytest.raises(TypeError):
        pkg.bicgstabl_batch_(np.zeros((4, 2), complex).T, A, np.ones((2, 4), complex))
    assert np.all(X == 0)
