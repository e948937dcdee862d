"""The ABI of lsfc_bicgstabl: the entry point exists in the built library, in include/lsfc.h and in _lib.py, the option
struct has the header's layout, and the argument checks that come before any device call answer without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fast_solver_lippmann_schwinger_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lsfc.h")
FIELDS = ["l", "max_mv_products", "reltol", "abstol", "initially_zero", "precond", "precond_user", "precond_on_device",
          "r_shadow", "reserved"]


def test_symbol_in_the_library_and_the_binding():
    fn = L.load().lsfc_bicgstabl
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    proto = re.search(r"\bint\s+lsfc_bicgstabl\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
    assert len(proto.split(",")) == 8 and "lsfc_bicgstabl_opts" in proto and "lsfc_gmres_result" in proto
    import fast_solver_lippmann_schwinger_amd as pkg
    assert callable(pkg.bicgstabl_) and "bicgstabl_" in pkg.__all__


def test_struct_layout_matches_the_header(tmp_path):
    assert [f[0] for f in L.BicgstablOpts._fields_] == FIELDS
    lines = ['#include <cstddef>', '#include "lsfc.h"',
             f'static_assert(sizeof(lsfc_bicgstabl_opts) == {C.sizeof(L.BicgstablOpts)}, "sizeof");']
    row = [f"size={C.sizeof(L.BicgstablOpts)}"]
    for name in FIELDS:
        off = getattr(L.BicgstablOpts, name).offset
        lines.append(f'static_assert(offsetof(lsfc_bicgstabl_opts, {name}) == {off}, "{name}");')
        row.append(f"{name}:{off}")
    lines.append(f'static_assert(sizeof(((lsfc_bicgstabl_opts*)0)->reserved) == {4 * C.sizeof(C.c_int)}, "reserved");')
    src = tmp_path / "abi_bicgstabl.cpp"
    src.write_text("\n".join(lines) + "\nint main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    # the Julia binding quotes the same offsets and lists the same fields in the same order
    jl = open(os.path.join(ROOT, "julia", "FastConvHIP.jl")).read()
    assert "# ABI-LAYOUT lsfc_bicgstabl_opts " + " ".join(row) in jl, " ".join(row)
    body = re.search(r"struct BicgstablOpts\n(.*?)\nend", jl, flags=re.S).group(1)
    assert re.findall(r"(\w+)::", body) == FIELDS
    assert "function bicgstabl_hip!" in jl


def test_argument_checks_before_any_device_call():
    # (no plan can exist without a GPU: the checks on opts and memspace come first and do not look at the plan)
    lib = L.load()
    x, b = np.zeros(4, complex), np.ones(4, complex)
    px, pb = x.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    res = L.GmresResult()

    def call(opts, plan=None, memspace=L.LSFC_MEM_HOST, x=px, result=C.byref(res)):
        rc = lib.lsfc_bicgstabl(plan, x, pb, opts, None, 0, result, memspace)
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
    rc, msg = call(C.byref(L.BicgstablOpts(l=2)), memspace=2)
    assert rc == L.LSFC_EINVAL and "memspace" in msg
    rc, msg = call(C.byref(L.BicgstablOpts(l=2)))                       # NULL plan
    assert rc == L.LSFC_EINVAL and "NULL argument" in msg
    assert np.all(x == 0)


def test_enomem_message_format():
    # the check itself needs a device; its message is part of the interface (figures as in lsfc_gmres_batch)
    src = open(os.path.join(ROOT, "fast_solver_lippmann_schwinger_amd", "csrc", "bicgstab.hip")).read()
    m = re.search(r'fail\(LSFC_ENOMEM, "([^"]*)"\s*"([^"]*)"', src, flags=re.S)
    assert m, "lsfc_bicgstabl: no LSFC_ENOMEM message"
    msg = m.group(1) + m.group(2)
    assert "2 l + 3" in msg and "GB of device memory" in msg and "GB are free" in msg
    # inside the entry point the check comes before the solver (which allocates the work vectors) and before the staging
    body = src[src.index('extern "C" int lsfc_bicgstabl'):]
    assert body.index("hipMemGetInfo") < body.index("plan->xs.alloc") < body.index("bicgstabl_run(")
    assert "work.alloc" in src[:src.index('extern "C" int lsfc_bicgstabl')]        # the only N-sized allocation of the solver
