"""CPU tests of the Born operator's reciprocal mode, in the manner of tests/test_abi_born.py: the new entry points are declared,
exported and bound; the two mode constants exist; every refusal that needs no object is LSFC_EINVAL before any device call, and
lsfc_last_error names the cause; the Python constructor refuses an unknown mode.  The refused calls never look behind a pointer;
what needs objects is checked in tests/test_gpu_born_reciprocal.py."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import fast_solver_lippmann_schwinger_amd as pkg
import fast_solver_lippmann_schwinger_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"lsfc_born_contract": 13, "lsfc_born_set_mode": 2, "lsfc_born_get_mode": 3, "lsfc_born_receiver_fields": 3, "lsfc_born_receiver_info": 3}

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
    for name, value in (("LSFC_BORN_ADJOINT_STATE", 0), ("LSFC_BORN_RECIPROCAL", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(L, name) == value
    assert "born_contract" in pkg.__all__ and callable(pkg.born_contract)
    # the option struct is what it was: the switch is a call, not a field
    assert [f for f, _ in L.BornOpts._fields_] == ["solver", "restart", "l", "maxiter", "reltol", "abstol", "precond", "chunk", "reserved"]
    assert "recycled Krylov spaces" in text
    julia = open(os.path.join(ROOT, "julia", "FastConvHIP.jl")).read()
    for word in ("set_mode!", "receiver_fields", "lsfc_born_contract"):
        assert word in julia, word
    assert "born_contract.hip" in open(os.path.join(ROOT, "README.md")).read()


def test_contract_refuses_bad_arguments_before_any_device_call():
    lib = L.load()
    H, N_, T_, H_ = L.LSFC_MEM_HOST, L.LSFC_OP_N, L.LSFC_OP_T, L.LSFC_OP_H
    # lsfc_born_contract(plan, u, nsrc, v, nrecv, in, in_is_complex, out, op, flags, scale_re, scale_im, memspace)
    ok = [OBJ, PBUF, 1, PBUF, 1, PBUF, 1, PBUF, N_, 0, 1.0, 0.0, H]
    for i in (0, 1, 3, 5, 7):
        args = list(ok)
        args[i] = None
        assert lib.lsfc_born_contract(*args) == L.LSFC_EINVAL and "NULL" in _err()

    def refused(word, **kw):
        args = list(ok)
        for name, value in kw.items():
            args[{"nsrc": 2, "nrecv": 4, "cplx": 6, "op": 8, "flags": 9, "memspace": 12}[name]] = value
        assert lib.lsfc_born_contract(*args) == L.LSFC_EINVAL and word in _err(), (kw, _err())

    refused("nsrc = 0", nsrc=0)
    refused("nrecv = -1", nrecv=-1)
    refused("bad op 3", op=3)
    refused("bad op -1", op=-1)
    refused("LSFC_OP_T is not offered", op=T_)
    refused("unknown flag", op=H_, flags=4)
    refused("go with LSFC_OP_H", flags=L.LSFC_BORN_REAL)
    refused("go with LSFC_OP_H", flags=L.LSFC_BORN_ACCUMULATE)
    refused("in_is_complex = 2", cplx=2)
    refused("nsrc x nrecv complex", op=H_, cplx=0)
    refused("memspace 2", memspace=2)
    assert np.all(BUF == 0)


def test_the_object_entries_refuse_bad_arguments_before_any_device_call():
    lib = L.load()
    for mode in (-1, 2, 7):
        assert lib.lsfc_born_set_mode(OBJ, mode) == L.LSFC_EINVAL and f"unknown mode {mode}" in _err()
    for mode in (L.LSFC_BORN_ADJOINT_STATE, L.LSFC_BORN_RECIPROCAL):
        assert lib.lsfc_born_set_mode(None, mode) == L.LSFC_EINVAL and "NULL" in _err()
    m, nbytes = C.c_int(-7), C.c_int64(-7)
    assert lib.lsfc_born_get_mode(None, C.byref(m), C.byref(nbytes)) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_get_mode(OBJ, None, C.byref(nbytes)) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_get_mode(OBJ, C.byref(m), None) == L.LSFC_EINVAL and "NULL" in _err()
    assert (m.value, nbytes.value) == (-7, -7)
    p, n = C.c_void_p(), C.c_int64(-7)
    assert lib.lsfc_born_receiver_fields(None, C.byref(p), C.byref(n)) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_receiver_fields(OBJ, None, C.byref(n)) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_receiver_fields(OBJ, C.byref(p), None) == L.LSFC_EINVAL and "NULL" in _err()
    assert p.value is None and n.value == -7
    assert lib.lsfc_born_receiver_info(None, (C.c_int64 * 4)(), None) == L.LSFC_EINVAL and "NULL" in _err()
    assert lib.lsfc_born_receiver_info(OBJ, None, None) == L.LSFC_EINVAL and "NULL" in _err()


def test_python_checks_the_mode_and_the_contraction_arguments():
    M = types.SimpleNamespace(shape=(8, 8), _plan=None, set_nu=None)
    R = pkg.Receivers.__new__(pkg.Receivers)                # (no device: the constructor's checks look at the type, N and nrecv only)
    R.N, R.nrecv, R._rc = 8, 2, None
    U = np.zeros((1, 8), complex)
    for mode in ("recip", None, 1):
        with pytest.raises(ValueError, match="mode must be"):
            pkg.BornOperator(M, R, U, mode=mode)
    with pytest.raises(ValueError, match="op must be"):
        pkg.born_contract(M, U, U, np.zeros(8), op="T")
    with pytest.raises(ValueError, match="go with op='H'"):
        pkg.born_contract(M, U, U, np.zeros(8), op="N", real=True)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.born_contract(M, np.zeros((1, 9), complex), U, np.zeros(8))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        pkg.born_contract(M, U, U, np.zeros(7))
