"""CPU: the native MADS driver's swarm-constraint entry points (mac_mads_run_cons,
mac_mads_begin_cons; include/maxcover.h) are exported and bound and fail cleanly without a context,
and FullSimulation.split_cons_ext turns the reference's ``cons_ext`` slot into the one mac_cons the
driver takes."""
import ctypes

import numpy as np
import pytest

MADS_CONS_SYMBOLS = ("mac_mads_run_cons", "mac_mads_begin_cons")
FOV = 100 / 180 * np.pi


def test_symbols_exported_and_bound(pkg):
    L = pkg.load_library()
    for s in MADS_CONS_SYMBOLS:
        assert s in pkg._lib.EXPORTS
        f = getattr(L, s)
        assert f.restype is ctypes.c_int32
        assert f.argtypes[-1] == ctypes.POINTER(pkg._lib.Cons)   # the trailing const mac_cons*
    # the existing argument lists plus the trailing pointer
    assert L.mac_mads_run_cons.argtypes[:-1] == L.mac_mads_run.argtypes
    assert L.mac_mads_begin_cons.argtypes[:-1] == L.mac_mads_begin.argtypes
    assert "cons_mask_gen_kernel" in pkg._lib.PROF_ROLES


def test_null_arguments_are_inval_without_a_gpu(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    dp = ctypes.POINTER(ctypes.c_double)
    cons = lib.Cons(15.0, float("nan"), float("nan"))
    x0 = np.array([0.0, 20.0, 0.0, 0.0, 5.0, 5.0])
    rm = np.ones(2)
    out = np.full(6, 7.0)
    prm = lib.MadsParams(3, 2, 5, 1)
    st = lib.MadsStats()
    st.iterations = 99
    xp, rp, op = x0.ctypes.data_as(dp), rm.ctypes.data_as(dp), out.ctypes.data_as(dp)
    for cp in (ctypes.byref(cons), None):   # a constraint on, and the plain call's forward
        # null context
        rc = L.mac_mads_run_cons(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), op,
                                 ctypes.byref(st), cp)
        assert rc == lib.MAC_E_INVAL
        assert "null" in L.mac_last_error().decode()
        # null x_out
        rc = L.mac_mads_run_cons(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), None,
                                 ctypes.byref(st), cp)
        assert rc == lib.MAC_E_INVAL
        h = ctypes.c_void_p(1234)
        rc = L.mac_mads_begin_cons(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 12,
                                   ctypes.byref(h), cp)
        assert rc == lib.MAC_E_INVAL and not h.value   # (the handle is cleared)
        # null out
        rc = L.mac_mads_begin_cons(None, xp, 6, rp, 1e5, None, None, 1.0, ctypes.byref(prm), 0, 12,
                                   None, cp)
        assert rc == lib.MAC_E_INVAL
    assert np.all(out == 7.0) and st.iterations == 99


def test_split_cons_ext(pkg):
    TC = pkg.TDM_Constraints
    split = pkg.FullSimulation.split_cons_ext
    assert split(()) is None and split(None) is None
    assert split([TC.cons1]) is None                       # cons1 (always true) is dropped
    c8, c7 = TC.create_cons8(15.0), TC.create_cons7(FOV, 200.0, 19.0)
    assert split([c8]) == {"d_sep": 15.0}
    assert split(c8) == {"d_sep": 15.0}                    # a single callable, as the reference passes
    m = split([TC.cons1, c8, c7])
    assert m == {"d_sep": 15.0, "zone_y": 200.0, "zone_r": 19.0 * np.tan(FOV / 2)}
    cs = pkg._lib.make_cons(m)                             # what Context.mads_run hands the library
    assert (cs.d_sep, cs.zone_y, cs.zone_r) == (15.0, 200.0, 19.0 * np.tan(FOV / 2))
    with pytest.raises(ValueError, match="lambda"):
        split([c8, lambda x: True])

    def my_rule(x):
        return True

    with pytest.raises(ValueError, match="my_rule"):
        split([my_rule])
    with pytest.raises(ValueError, match="cons8"):         # two of one kind: one slot
        split([c8, TC.create_cons8(10.0)])


def test_simulation_rejects_a_host_only_constraint_before_touching_the_context(pkg):
    with pytest.raises(ValueError, match="native MADS driver"):
        pkg.FullSimulation.Simulation(None, np.zeros(6), initial_points=np.zeros((0, 5)),
                                      cons_ext=[lambda x: True])
