"""CPU: the native MADS driver's mesh entry points (mac_mads_run_mesh, mac_mads_begin_mesh,
mac_mads_mesh; include/maxcover.h) are exported and bound, fail cleanly without a context, and
reject a bad mesh with a message of their own before anything is written."""
import ctypes
import math

import numpy as np
import pytest

MESH_SYMBOLS = ("mac_mads_run_mesh", "mac_mads_begin_mesh")


def test_symbols_exported_and_bound(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    for s in MESH_SYMBOLS:
        assert s in lib.EXPORTS
        f = getattr(L, s)
        assert f.restype is ctypes.c_int32
        assert f.argtypes[-1] == ctypes.POINTER(lib.MadsMesh)   # the trailing const mac_mads_mesh*
    # the _motion argument lists plus the trailing pointer
    assert L.mac_mads_run_mesh.argtypes[:-1] == L.mac_mads_run_motion.argtypes
    assert L.mac_mads_begin_mesh.argtypes[:-1] == L.mac_mads_begin_motion.argtypes
    assert ctypes.sizeof(lib.MadsMesh) == 16
    assert lib.MadsMesh.granularity.offset == 0 and lib.MadsMesh.reserved.offset == 8
    assert ctypes.sizeof(lib.MadsOpts) == 16   # (mac_mads_opts is what it was)


def _args(lib):
    dp = ctypes.POINTER(ctypes.c_double)
    x0 = np.array([0.0, 20.0, 0.0, 0.0, 5.0, 5.0])
    rm = np.ones(2)
    out = np.full(6, 7.0)
    prm = lib.MadsParams(3, 2, 5, 1)
    st = lib.MadsStats()
    st.iterations = 99
    return x0, rm, out, prm, st, x0.ctypes.data_as(dp), rm.ctypes.data_as(dp), out.ctypes.data_as(dp)


def _mesh(lib, g, reserved=0):
    g = None if g is None else np.ascontiguousarray(g, dtype=np.float64)
    m = lib.MadsMesh(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if g is not None else None, reserved)
    return m, g   # (g kept alive by the caller)


def test_null_context_is_inval_without_a_gpu(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    x0, rm, out, prm, st, xp, rp, op = _args(lib)
    xy = lib.MadsOpts(lib.MAC_POLL_XY)
    meshes = [_mesh(lib, None), _mesh(lib, np.ones(6)), _mesh(lib, [1.0, 1.0, 1.0, 1.0, 0.1, 0.125]),
              _mesh(lib, np.full(6, 0.5))]
    for mp in [None] + [ctypes.byref(m) for m, _ in meshes]:
        for o in (None, ctypes.byref(xy)):
            rc = L.mac_mads_run_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), op,
                                     ctypes.byref(st), None, o, None, mp)
            assert rc == lib.MAC_E_INVAL
            assert "null" in L.mac_last_error().decode()
            rc = L.mac_mads_run_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), None,
                                     ctypes.byref(st), None, o, None, mp)   # null x_out
            assert rc == lib.MAC_E_INVAL
            h = ctypes.c_void_p(1234)
            rc = L.mac_mads_begin_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 8,
                                       ctypes.byref(h), None, o, None, mp)
            assert rc == lib.MAC_E_INVAL and not h.value   # (the handle is cleared)
            assert "null" in L.mac_last_error().decode()
            rc = L.mac_mads_begin_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 8,
                                       None, None, o, None, mp)              # null out
            assert rc == lib.MAC_E_INVAL
    assert np.all(out == 7.0) and st.iterations == 99


@pytest.mark.parametrize("bad", ["zero", "negative", "nan", "inf", "neg_inf", "last_entry", "radius_under_xy",
                                 "reserved", "reserved_null_vector"])
def test_a_bad_mesh_is_inval_with_its_own_message(pkg, bad):
    L = pkg.load_library()
    lib = pkg._lib
    x0, rm, out, prm, st, xp, rp, op = _args(lib)
    g = np.array([1.0, 0.5, 1.0, 2.0, 0.1, 0.125])
    reserved, opts = 0, None
    if bad in ("zero", "negative", "nan", "inf", "neg_inf"):
        g[1] = {"zero": 0.0, "negative": -1.0, "nan": math.nan, "inf": math.inf, "neg_inf": -math.inf}[bad]
    elif bad == "last_entry":
        g[5] = 0.0
    elif bad == "radius_under_xy":   # (unused by an xy-only poll, validated all the same)
        g[4] = -0.0
        opts = lib.MadsOpts(lib.MAC_POLL_XY)
    elif bad == "reserved":
        reserved = 1
    else:
        g, reserved = None, 1
    m, keep = _mesh(lib, g, reserved)
    o = ctypes.byref(opts) if opts is not None else None
    rc = L.mac_mads_run_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), op,
                             ctypes.byref(st), None, o, None, ctypes.byref(m))
    assert rc == lib.MAC_E_INVAL
    assert "mac_mads_mesh" in L.mac_last_error().decode()   # (the mesh's own message, not "null")
    h = ctypes.c_void_p(1234)
    rc = L.mac_mads_begin_mesh(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 12,
                               ctypes.byref(h), None, o, None, ctypes.byref(m))
    assert rc == lib.MAC_E_INVAL and not h.value
    assert "mac_mads_mesh" in L.mac_last_error().decode()
    assert np.all(out == 7.0) and st.iterations == 99


def test_fused_hint_read_out_is_exported_and_fails_cleanly(pkg):
    """mac_profile_fused (the fused chain's hint word 1, read by tools/mads_granularity_time.py)."""
    L = pkg.load_library()
    lib = pkg._lib
    assert "mac_profile_fused" in lib.EXPORTS
    assert L.mac_profile_fused.restype is ctypes.c_int32
    r = ctypes.c_int64(7)
    assert L.mac_profile_fused(None, ctypes.byref(r), None, None, 0) == lib.MAC_E_INVAL
    assert "null" in L.mac_last_error().decode() and r.value == 7
