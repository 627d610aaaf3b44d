"""CPU: the native MADS driver's poll-kind entry points (mac_mads_run_opts, mac_mads_begin_opts,
mac_mads_opts; include/maxcover.h) are exported and bound and fail cleanly without a context, and
FullSimulation.Simulation's ``poll_vars`` keyword validates and decides "auto" on the host."""
import ctypes
import math

import numpy as np
import pytest

OPTS_SYMBOLS = ("mac_mads_run_opts", "mac_mads_begin_opts")
TAN50 = math.tan(100 / 180 * math.pi / 2)


def test_symbols_exported_and_bound(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    for s in OPTS_SYMBOLS:
        assert s in lib.EXPORTS
        f = getattr(L, s)
        assert f.restype is ctypes.c_int32
        assert f.argtypes[-1] == ctypes.POINTER(lib.MadsOpts)   # the trailing const mac_mads_opts*
    # the _cons argument lists plus the trailing pointer
    assert L.mac_mads_run_opts.argtypes[:-1] == L.mac_mads_run_cons.argtypes
    assert L.mac_mads_begin_opts.argtypes[:-1] == L.mac_mads_begin_cons.argtypes
    assert ctypes.sizeof(lib.MadsOpts) == 16
    assert (lib.MAC_POLL_XYR, lib.MAC_POLL_XY) == (0, 1)
    assert lib.POLL_VARS == {"xyr": 0, "xy": 1}


def _args(lib):
    dp = ctypes.POINTER(ctypes.c_double)
    x0 = np.array([0.0, 20.0, 0.0, 0.0, 5.0, 5.0])
    rm = np.ones(2)
    out = np.full(6, 7.0)
    prm = lib.MadsParams(3, 2, 5, 1)
    st = lib.MadsStats()
    st.iterations = 99
    return x0, rm, out, prm, st, x0.ctypes.data_as(dp), rm.ctypes.data_as(dp), out.ctypes.data_as(dp)


def test_null_arguments_are_inval_without_a_gpu(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    x0, rm, out, prm, st, xp, rp, op = _args(lib)
    cons = lib.Cons(15.0, float("nan"), float("nan"))
    xyr, xy = lib.MadsOpts(lib.MAC_POLL_XYR), lib.MadsOpts(lib.MAC_POLL_XY)
    for o in (None, ctypes.byref(xyr), ctypes.byref(xy)):
        for cp in (ctypes.byref(cons), None):
            # null context
            rc = L.mac_mads_run_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), op,
                                     ctypes.byref(st), cp, o)
            assert rc == lib.MAC_E_INVAL
            assert "null" in L.mac_last_error().decode()
            # null x_out
            rc = L.mac_mads_run_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), None,
                                     ctypes.byref(st), cp, o)
            assert rc == lib.MAC_E_INVAL
            h = ctypes.c_void_p(1234)
            rc = L.mac_mads_begin_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 8,
                                       ctypes.byref(h), cp, o)
            assert rc == lib.MAC_E_INVAL and not h.value   # (the handle is cleared)
            # null out
            rc = L.mac_mads_begin_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 8,
                                       None, cp, o)
            assert rc == lib.MAC_E_INVAL
    assert np.all(out == 7.0) and st.iterations == 99


@pytest.mark.parametrize("bad", ["poll_vars", "reserved0", "reserved2"])
def test_unknown_options_are_inval(pkg, bad):
    L = pkg.load_library()
    lib = pkg._lib
    x0, rm, out, prm, st, xp, rp, op = _args(lib)
    o = lib.MadsOpts(lib.MAC_POLL_XY)
    if bad == "poll_vars":
        o.poll_vars = 7
    else:
        o.reserved[int(bad[-1])] = 1
    rc = L.mac_mads_run_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), op,
                             ctypes.byref(st), None, ctypes.byref(o))
    assert rc == lib.MAC_E_INVAL
    assert "mac_mads_opts" in L.mac_last_error().decode()   # (the options' own message, not "null")
    h = ctypes.c_void_p(1234)
    rc = L.mac_mads_begin_opts(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 8,
                               ctypes.byref(h), None, ctypes.byref(o))
    assert rc == lib.MAC_E_INVAL and not h.value
    assert "mac_mads_opts" in L.mac_last_error().decode()
    assert np.all(out == 7.0) and st.iterations == 99


def test_python_keywords_validate_before_the_library(pkg):
    lib = pkg._lib
    assert lib.poll_vars_code("xyr") == 0 and lib.poll_vars_code("xy") == 1
    for v in ("z", "auto", None, 1):
        with pytest.raises(ValueError, match="poll_vars"):
            lib.poll_vars_code(v)
    TS = pkg.TDM_STATIC_opt
    assert TS.polled_count(36) == 36 and TS.polled_count(36, "xy") == 24
    with pytest.raises(ValueError, match="poll_vars"):
        TS.polled_count(36, "z")
    with pytest.raises(ValueError, match="poll_vars"):
        TS.mads(np.zeros(6), lambda v: 0.0, poll_vars="z")


def test_simulation_rejects_an_unknown_poll_kind_before_touching_the_context(pkg):
    with pytest.raises(ValueError, match="poll_vars"):
        pkg.FullSimulation.Simulation(None, np.zeros(6), initial_points=np.zeros((0, 5)), poll_vars="z")


def test_auto_rule_on_hand_made_radii(pkg):
    """"xy" iff every |R_i - r_max_i| <= 0.5: at 0.5 exactly, just below and just above, either
    side of r_max, and one UAV off among many on."""
    auto = pkg.FullSimulation.auto_poll_vars
    r_max = np.array([30.0 * TAN50, 15.0 * TAN50, 36.0])
    assert auto(r_max.copy(), r_max) == "xy"
    rm = np.array([36.0, 36.0, 20.0])                       # (exact doubles: 0.5 is representable)
    assert auto(rm + 0.5, rm) == "xy" and auto(rm - 0.5, rm) == "xy"
    # the neighbouring doubles of r_max +- 0.5 (the differences are exact: Sterbenz)
    assert auto(np.nextafter(rm + 0.5, rm), rm) == "xy" and auto(np.nextafter(rm - 0.5, rm), rm) == "xy"
    for i in range(3):
        for sg in (1.0, -1.0):
            R = rm.copy()
            R[i] = np.nextafter(rm[i] + sg * 0.5, sg * np.inf)
            assert abs(R[i] - rm[i]) > 0.5
            assert auto(R, rm) == "xyr"
    assert auto(np.array([36.0, 36.0, 26.0]), rm) == "xyr"
    assert auto(np.array([36.0, np.nan, 20.0]), rm) == "xyr"   # (not known to be in place)
