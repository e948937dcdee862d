"""CPU tests of lsfc_born_*: the entry points are declared, exported and bound; every refusal that needs no object is LSFC_EINVAL
before any device call, and lsfc_last_error names the cause; the Python constructor's own checks.  Without a device no plan and no
receivers object can exist (their creators answer LSFC_ENODEV), so the refused calls are built so that they never look behind a
pointer; what needs objects is checked in tests/test_gpu_born.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import fast_solver_lippmann_schwinger_amd as pkg
import fast_solver_lippmann_schwinger_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lsfc_born_scale": 7, "lsfc_born_image": 9, "lsfc_born_create": 4, "lsfc_born_destroy": 1, "lsfc_born_set_background": 4,
         "lsfc_born_fields": 3, "lsfc_born_data": 3, "lsfc_born_apply": 7, "lsfc_born_info": 3}

STAND_IN = (C.c_char * 4096)()                              # a non-NULL object address that is never read
OBJ = C.cast(STAND_IN, C.c_void_p)
BUF = np.zeros(64, dtype=np.complex128)
PBUF = BUF.ctypes.data_as(C.c_void_p)


def _err():
    return L.load().lsfc_last_error().decode()


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "lsfc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = dict(re.findall(r"\b(lsfc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S))
    lib = C.CDLL(L.LIB_PATH)
    for name, nparams in NAMES.items():
        assert name in protos, f"{name} not declared"
        assert hasattr(lib, name), f"{name} not exported"
        assert len([a for a in protos[name].split(",") if a.strip()]) == nparams == len(L.SIGNATURES[name][1]), name
    for name, value in (("LSFC_BORN_ACCUMULATE", 1), ("LSFC_BORN_REAL", 2), ("LSFC_BORN_GMRES", 0), ("LSFC_BORN_BICGSTABL", 1)):
        assert re.search(r"#define\s+%s\s+%du?\b" % (name, value), text), name
        assert getattr(L, name) == value
    assert "BornOperator" in pkg.__all__ and callable(pkg.BornOperator)
    # "gradient assembly" is no longer out of scope anywhere
    for doc in ("include/lsfc.h", "README.md", "DESIGN.md"):
        assert "gradient assembly" not in open(os.path.join(ROOT, doc)).read(), doc
    assert "struct Born" in open(os.path.join(ROOT, "julia", "FastConvHIP.jl")).read()


def test_the_option_struct_matches_the_header(tmp_path):
    import subprocess
    lines = ['#include <cstddef>', '#include "lsfc.h"', f'static_assert(sizeof(lsfc_born_opts) == {C.sizeof(L.BornOpts)}, "size");']
    for fname, _ in L.BornOpts._fields_:
        lines.append(f'static_assert(offsetof(lsfc_born_opts, {fname}) == {getattr(L.BornOpts, fname).offset}, "{fname}");')
    src = tmp_path / "born_opts.cpp"
    src.write_text("\n".join(lines) + "\nint main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def test_kernel_entries_refuse_bad_arguments_before_any_device_call():
    lib = L.load()
    H = L.LSFC_MEM_HOST
    # lsfc_born_scale(plan, dnu, dnu_is_complex, u, out, nrhs, memspace)
    for args in ((None, PBUF, 0, PBUF, PBUF, 1, H), (OBJ, None, 0, PBUF, PBUF, 1, H), (OBJ, PBUF, 0, None, PBUF, 1, H), (OBJ, PBUF, 0, PBUF, None, 1, H)):
        assert lib.lsfc_born_scale(*args) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_scale(OBJ, PBUF, 2, PBUF, PBUF, 1, H) == L.LSFC_EINVAL and "dnu_is_complex = 2" in _err()
    assert lib.lsfc_born_scale(OBJ, PBUF, 0, PBUF, PBUF, 0, H) == L.LSFC_EINVAL and "nrhs = 0" in _err()
    assert lib.lsfc_born_scale(OBJ, PBUF, 0, PBUF, PBUF, 1, 2) == L.LSFC_EINVAL and "memspace 2" in _err()
    # lsfc_born_image(plan, u, p, nrhs, scale_re, scale_im, flags, g, memspace)
    for args in ((None, PBUF, PBUF, 1, 1.0, 0.0, 0, PBUF, H), (OBJ, None, PBUF, 1, 1.0, 0.0, 0, PBUF, H), (OBJ, PBUF, None, 1, 1.0, 0.0, 0, PBUF, H),
                 (OBJ, PBUF, PBUF, 1, 1.0, 0.0, 0, None, H)):
        assert lib.lsfc_born_image(*args) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_image(OBJ, PBUF, PBUF, -1, 1.0, 0.0, 0, PBUF, H) == L.LSFC_EINVAL and "nrhs = -1" in _err()
    assert lib.lsfc_born_image(OBJ, PBUF, PBUF, 1, 1.0, 0.0, 4, PBUF, H) == L.LSFC_EINVAL and "unknown flag" in _err()
    assert lib.lsfc_born_image(OBJ, PBUF, PBUF, 1, 1.0, 0.0, 0, PBUF, 3) == L.LSFC_EINVAL and "memspace 3" in _err()
    assert np.all(BUF == 0)


def test_create_refuses_bad_arguments_before_any_device_call():
    lib = L.load()
    b = C.c_void_p()
    ok = L.BornOpts(solver=L.LSFC_BORN_GMRES, l=2)
    for args in ((None, OBJ, OBJ, C.byref(ok)), (C.byref(b), None, OBJ, C.byref(ok)), (C.byref(b), OBJ, None, C.byref(ok)), (C.byref(b), OBJ, OBJ, None)):
        assert lib.lsfc_born_create(*args) == L.LSFC_EINVAL and "NULL" in _err()
    for i in range(6):
        o = L.BornOpts(solver=L.LSFC_BORN_GMRES)
        o.reserved[i] = 3
        assert lib.lsfc_born_create(C.byref(b), OBJ, OBJ, C.byref(o)) == L.LSFC_EINVAL and f"reserved[{i}]" in _err()
    for solver in (-1, 2):
        assert lib.lsfc_born_create(C.byref(b), OBJ, OBJ, C.byref(L.BornOpts(solver=solver))) == L.LSFC_EINVAL
        assert f"unknown solver {solver}" in _err()
    for l in (0, 9):
        assert lib.lsfc_born_create(C.byref(b), OBJ, OBJ, C.byref(L.BornOpts(solver=L.LSFC_BORN_BICGSTABL, l=l))) == L.LSFC_EINVAL
        assert "1..8" in _err()
    assert lib.lsfc_born_create(C.byref(b), OBJ, OBJ, C.byref(L.BornOpts(solver=0, chunk=65))) == L.LSFC_EINVAL and "chunk = 65" in _err()
    assert b.value is None


def test_the_object_entries_refuse_bad_arguments_before_any_device_call():
    lib = L.load()
    H, N_, T_, H_ = L.LSFC_MEM_HOST, L.LSFC_OP_N, L.LSFC_OP_T, L.LSFC_OP_H
    # lsfc_born_apply(b, in, in_is_complex, out, op, flags, memspace)
    for args in ((None, PBUF, 1, PBUF, N_, 0, H), (OBJ, None, 1, PBUF, N_, 0, H), (OBJ, PBUF, 1, None, N_, 0, H)):
        assert lib.lsfc_born_apply(*args) == L.LSFC_EINVAL and "NULL" in _err()
    for op in (-1, 3):
        assert lib.lsfc_born_apply(OBJ, PBUF, 1, PBUF, op, 0, H) == L.LSFC_EINVAL and f"bad op {op}" in _err()
    assert lib.lsfc_born_apply(OBJ, PBUF, 1, PBUF, T_, 0, H) == L.LSFC_EINVAL and "LSFC_OP_T is not offered" in _err()
    for flags in (1, 4, 6):
        assert lib.lsfc_born_apply(OBJ, PBUF, 1, PBUF, H_, flags, H) == L.LSFC_EINVAL and "unknown flag" in _err()
    assert lib.lsfc_born_apply(OBJ, PBUF, 1, PBUF, N_, L.LSFC_BORN_REAL, H) == L.LSFC_EINVAL and "LSFC_BORN_REAL goes with LSFC_OP_H" in _err()
    assert lib.lsfc_born_apply(OBJ, PBUF, 2, PBUF, N_, 0, H) == L.LSFC_EINVAL and "in_is_complex = 2" in _err()
    assert lib.lsfc_born_apply(OBJ, PBUF, 0, PBUF, H_, 0, H) == L.LSFC_EINVAL and "residuals" in _err()
    assert lib.lsfc_born_apply(OBJ, PBUF, 1, PBUF, N_, 0, 2) == L.LSFC_EINVAL and "memspace 2" in _err()
    # the others
    assert lib.lsfc_born_set_background(None, PBUF, 1, H) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_set_background(OBJ, None, 1, H) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_set_background(OBJ, PBUF, 0, H) == L.LSFC_EINVAL and "nsrc = 0" in _err()
    assert lib.lsfc_born_set_background(OBJ, PBUF, 1, 5) == L.LSFC_EINVAL and "memspace 5" in _err()
    p, n = C.c_void_p(), C.c_int64(-7)
    assert lib.lsfc_born_fields(None, C.byref(p), C.byref(n)) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_fields(OBJ, None, C.byref(n)) == L.LSFC_EINVAL and n.value == -7
    assert lib.lsfc_born_data(None, PBUF, H) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_data(OBJ, None, H) == L.LSFC_EINVAL
    assert lib.lsfc_born_data(OBJ, PBUF, 2) == L.LSFC_EINVAL and "memspace 2" in _err()
    assert lib.lsfc_born_info(None, (C.c_int64 * 8)(), None) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_info(OBJ, None, None) == L.LSFC_EINVAL
    assert lib.lsfc_born_destroy(None) == 0
    assert np.all(BUF == 0)


def test_valid_arguments_reach_the_device():
    # A Born operator is a plan, a receivers object and options: with every argument in order the first device call is the plan's
    # creator.  With a GPU the whole chain builds; without one it ends there with LSFC_ENODEV ("no CPU fallback"), not LSFC_EINVAL.
    n = 6
    h = 1.0 / n
    x = -0.5 + h * np.arange(n)
    Xg, Yg, Zg = np.meshgrid(x, x, x, indexing="ij")
    X, Y, Z = (A.reshape(-1, order="F") for A in (Xg, Yg, Zg))
    nu = 0.1 * np.exp(-10 * (X ** 2 + Y ** 2 + Z ** 2))
    if pkg.device_count() > 0:
        M = pkg.buildFastConvolution3D(x, x, x, X, Y, Z, h, 3.0, nu)
        R = pkg.Receivers(x, x, x, k=3.0, directions=[[0.0, 0.6, 0.8]])
        B = pkg.BornOperator(M, R, np.exp(3j * X)[None, :])
        assert B.converged and B.data.shape == (1, 1)
        B.close()
    else:
        with pytest.raises(L.LsfcError) as e:
            pkg.buildFastConvolution3D(x, x, x, X, Y, Z, h, 3.0, nu)
        assert e.value.code == L.LSFC_ENODEV and "no CPU fallback" in str(e.value)


def test_python_constructor_checks_its_arguments():
    M = types.SimpleNamespace(shape=(8, 8), _plan=None, set_nu=None)
    view = types.SimpleNamespace(shape=(8, 8), _plan=None, _op=L.LSFC_OP_T, parent=M)
    U = np.zeros((1, 8), complex)
    with pytest.raises(TypeError, match="not a view"):
        pkg.BornOperator(view, None, U)
    with pytest.raises(TypeError, match="Receivers"):
        pkg.BornOperator(M, object(), U)
    R = pkg.Receivers.__new__(pkg.Receivers)                # (no device: the constructor's checks look at the type, N and nrecv only)
    R.N, R.nrecv, R._rc = 8, 2, None
    with pytest.raises(TypeError, match="SparsifyingPreconditioner"):
        pkg.BornOperator(M, R, U, Pl=lambda v: None)
    with pytest.raises(ValueError, match="solver"):
        pkg.BornOperator(M, R, U, solver="cg")
    with pytest.raises(ValueError, match="chunk"):
        pkg.BornOperator(M, R, U, chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        pkg.BornOperator(M, R, U, chunk=65)
    R.N = 9
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.BornOperator(M, R, U)
