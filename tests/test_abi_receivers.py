"""CPU tests of lsfc_receivers_*: every argument error is LSFC_EINVAL before any device call, and lsfc_last_error names the
cause.  What needs an object (and so a device) is checked in test_gpu_receivers.py."""
import ctypes as C

import numpy as np
import pytest

import fast_solver_lippmann_schwinger_amd as pkg
import fast_solver_lippmann_schwinger_amd._lib as L


def _create(ndim=3, dims=(4, 5, 6), origin=(-0.3, -0.2, -0.1), h=0.125, k=5.0, kind=L.LSFC_RECV_POINTS, coords=None, nrecv=None,
            out=True, null=()):
    lib = L.load()
    if coords is None:
        coords = np.array([[2.0, 0.1, 0.3][:ndim], [-1.0, 0.5, 0.2][:ndim]])
        if kind == L.LSFC_RECV_FARFIELD:
            coords = coords / np.linalg.norm(coords, axis=1)[:, None]
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    rc = C.c_void_p()
    d = None if "dims" in null else (C.c_int64 * 3)(*dims)
    o = None if "origin" in null else (C.c_double * 3)(*origin)
    c = None if "coords" in null else coords.ctypes.data_as(C.c_void_p)
    code = lib.lsfc_receivers_create(C.byref(rc) if out else None, ndim, d, o, h, k, kind, c,
                                     coords.shape[0] if nrecv is None else nrecv, 0)
    return code, lib.lsfc_last_error().decode(), rc


def _expect(code_msg, *words):
    code, msg, rc = code_msg
    assert code == L.LSFC_EINVAL, (code, msg)
    assert rc.value is None
    for w in words:
        assert w in msg, msg


def test_create_null_arguments():
    _expect(_create(out=False), "NULL")
    for which in ("dims", "origin", "coords"):
        _expect(_create(null=(which,)), "NULL")


def test_create_bad_scalars():
    _expect(_create(ndim=1), "ndim = 1")
    _expect(_create(ndim=4), "ndim = 4")
    _expect(_create(dims=(4, 0, 6)), "dimension 1")
    _expect(_create(dims=(4, 5, -2)), "dimension 2")
    _expect(_create(ndim=2, dims=(0, 5, 1)), "dimension 0")
    _expect(_create(h=0.0), "h = 0")
    _expect(_create(h=-0.1), "h = -0.1")
    _expect(_create(k=0.0), "k = 0")
    _expect(_create(k=-3.0), "k = -3")
    _expect(_create(nrecv=0), "nrecv = 0")
    _expect(_create(nrecv=-1), "nrecv = -1")
    _expect(_create(kind=2), "kind 2")
    _expect(_create(kind=-1), "kind -1")


def test_far_field_direction_must_be_a_unit_vector():
    th = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [0.6, 0.8, 1e-5]])
    _expect(_create(kind=L.LSFC_RECV_FARFIELD, coords=th), "direction 2", "unit vector")
    th2 = np.array([[0.6 * (1 + 2e-11), 0.8]])
    _expect(_create(ndim=2, dims=(4, 5, 1), kind=L.LSFC_RECV_FARFIELD, coords=th2), "direction 0")


def test_point_receiver_on_a_grid_point_names_its_index():
    h, origin = 0.125, (-0.3, -0.2, -0.1)
    on = [origin[0] + 2 * h, origin[1] + 4 * h, origin[2] + 5 * h]                # a corner-ish grid point
    pts = np.array([[2.0, 0.1, 0.3], [0.01, 0.02, 0.03], on, [1.0, 1.0, 1.0]])
    _expect(_create(coords=pts), "receiver 2", "grid point")
    pts[2][0] += 0.5e-8 * h                                                         # still closer than 1e-8 h
    _expect(_create(coords=pts), "receiver 2")
    pts2 = np.array([[origin[0], origin[1] + 1e-9 * h]])
    _expect(_create(ndim=2, dims=(4, 5, 1), coords=pts2), "receiver 0")


def test_the_other_entry_points_refuse_null():
    lib = L.load()
    buf = (C.c_double * 8)()
    out6 = (C.c_int64 * 6)()
    assert lib.lsfc_receivers_apply(None, None, buf, buf, 1, L.LSFC_OP_N, L.LSFC_MEM_HOST) == L.LSFC_EINVAL
    assert "NULL" in lib.lsfc_last_error().decode()
    assert lib.lsfc_receivers_set_stream(None, None) == L.LSFC_EINVAL
    assert "NULL" in lib.lsfc_last_error().decode()
    assert lib.lsfc_receivers_info(None, out6) == L.LSFC_EINVAL
    assert "NULL" in lib.lsfc_last_error().decode()
    assert lib.lsfc_receivers_destroy(None) == 0


def test_valid_arguments_reach_the_device():
    # with every argument in order the call goes on to the device: an object with a GPU, LSFC_ENODEV ("no CPU fallback") without
    code, msg, rc = _create()
    if pkg.device_count() > 0:
        assert code == 0 and rc.value
        assert L.load().lsfc_receivers_destroy(rc) == 0
    else:
        assert code == L.LSFC_ENODEV and "no CPU fallback" in msg


def test_python_constructor_checks_its_axes():
    x = np.linspace(-0.5, 0.5, 9)
    with pytest.raises(ValueError):
        pkg.Receivers(x, x ** 3, k=3.0, directions=[[1.0, 0.0]])
    with pytest.raises(ValueError):
        pkg.Receivers(x, 2 * x, k=3.0, directions=[[1.0, 0.0]])
    with pytest.raises(ValueError):
        pkg.Receivers(x, x, k=3.0)
    with pytest.raises(ValueError):
        pkg.Receivers(x, x, k=3.0, points=[[2.0, 0.0]], directions=[[1.0, 0.0]])
    with pytest.raises(ValueError):
        pkg.Receivers(x, x, x, k=3.0, points=[[2.0, 0.0]])
    with pytest.raises(TypeError):
        pkg.Receivers(x, x, points=[[2.0, 0.0]])
