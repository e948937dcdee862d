"""CPU tests of the batched preconditioner entry points (lsfc_precond_apply_batch, lsfc_precond_batch_info): the header
and the ctypes binding declare them with matching prototypes, the library exports them, and their argument checks are
decided before any device call -- they answer LSFC_EINVAL on a machine without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"lsfc_precond_apply_batch": "ippli", "lsfc_precond_batch_info": "ipp"}    # return type, then parameters
LSFC_EINVAL = -1


def _header():
    text = open(os.path.join(ROOT, "include", "lsfc.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_and_binding_declare_the_new_entries():
    import fast_solver_lippmann_schwinger_amd._lib as L
    protos = dict(re.findall(r"\b(lsfc_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S))
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/lsfc.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} is not exported"
        nparams = len([a for a in protos[name].split(",") if a.strip()])
        assert nparams == len(L.SIGNATURES[name][1])
    assert re.search(r"int\s+lsfc_precond_apply_batch\s*\(\s*lsfc_precond\s*\*\s*pc\s*,\s*double\s*\*\s*v\s*,\s*int64_t\s+nrhs\s*,\s*int\s+memspace\s*\)",
                     _header())
    assert re.search(r"int\s+lsfc_precond_batch_info\s*\(\s*const\s+lsfc_precond\s*\*\s*pc\s*,\s*int64_t\s+out\s*\[\s*4\s*\]\s*\)", _header())


def test_prototypes_match_the_binding_types(tmp_path):
    # the static_assert scheme of tests/test_abi.py for the two new prototypes: class of the return type and of each parameter
    import fast_solver_lippmann_schwinger_amd._lib as L

    def cls(t):
        return {None: "v", C.c_int: "i", C.c_int64: "l", C.c_double: "d", C.c_uint: "u", C.c_size_t: "z"}.get(t, "p")
    lines = ['#include <cstddef>', '#include <cstdint>', '#include <type_traits>', '#include "lsfc.h"',
             'template <class T> constexpr char cls() {',
             '  if constexpr (std::is_void<T>::value) return \'v\'; else if constexpr (std::is_pointer<T>::value) return \'p\';',
             '  else if constexpr (std::is_same<T, int>::value) return \'i\'; else if constexpr (std::is_same<T, int64_t>::value) return \'l\';',
             '  else if constexpr (std::is_same<T, double>::value) return \'d\'; else return \'?\'; }',
             'template <class R, class... A> constexpr bool sig(R (*)(A...), const char* want) {',
             '  const char got[] = { cls<R>(), cls<A>()..., 0 };',
             '  for (int i = 0;; ++i) { if (got[i] != want[i]) return false; if (!got[i]) return true; } }']
    for name, want in NEW.items():
        res, args = L.SIGNATURES[name]
        assert cls(res) + "".join(cls(a) for a in args) == want, name
        lines.append(f'static_assert(sig(&{name}, "{want}"), "{name}: binding passes {want}");')
    src = tmp_path / "abi_batch.cpp"
    src.write_text("\n".join(lines) + "\nint main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def test_argument_checks_come_before_any_device_call():
    # No object can exist without a device, and none is needed: the refused calls never look behind the pointer.
    import fast_solver_lippmann_schwinger_amd._lib as L
    lib = L.load()
    v = np.zeros(8, dtype=np.complex128)
    pv = v.ctypes.data_as(C.c_void_p)
    stand_in = (C.c_char * 4096)()                                            # a non-NULL address that is never read
    pc = C.cast(stand_in, C.c_void_p)
    out4 = (C.c_int64 * 4)()
    assert lib.lsfc_precond_apply_batch(None, pv, 1, L.LSFC_MEM_HOST) == LSFC_EINVAL
    assert "NULL" in lib.lsfc_last_error().decode()
    assert lib.lsfc_precond_apply_batch(pc, None, 1, L.LSFC_MEM_HOST) == LSFC_EINVAL
    for nrhs in (0, -3):
        assert lib.lsfc_precond_apply_batch(pc, pv, nrhs, L.LSFC_MEM_HOST) == LSFC_EINVAL
        assert "nrhs" in lib.lsfc_last_error().decode()
    for space in (-1, 2, 7):
        assert lib.lsfc_precond_apply_batch(pc, pv, 1, space) == LSFC_EINVAL
        assert "memspace" in lib.lsfc_last_error().decode()
    assert lib.lsfc_precond_batch_info(None, out4) == LSFC_EINVAL
    assert lib.lsfc_precond_batch_info(pc, None) == LSFC_EINVAL
    assert np.all(v == 0) and bytes(stand_in) == bytes(4096)


def test_python_methods_exist_and_check_shapes_without_a_device():
    from fast_solver_lippmann_schwinger_amd.preconditioner import SparsifyingPreconditioner, BATCH_FIELDS
    assert BATCH_FIELDS == ("sweeps", "vectors", "largest_group", "work_bytes")
    for name in ("ldiv_batch_", "solve_batch", "batch_info"):
        assert callable(getattr(SparsifyingPreconditioner, name))
    P = SparsifyingPreconditioner.__new__(SparsifyingPreconditioner)          # no device object behind it
    P.N, P._pc = 6, None
    with pytest.raises(ValueError, match="DimensionMismatch"):
        P.ldiv_batch_(np.zeros((2, 7), dtype=np.complex128))
    with pytest.raises(ValueError, match="DimensionMismatch"):
        P.ldiv_batch_(np.zeros(6, dtype=np.complex128))
    with pytest.raises(TypeError, match="complex128"):
        P.ldiv_batch_(np.zeros((2, 6), dtype=np.float64))
    with pytest.raises(TypeError, match="complex128"):
        P.ldiv_batch_([[0j] * 6])
