"""CPU: the high-interest region entry points (mac_set_regions, mac_regions_ingested,
mac_region_stats_f64; include/maxcover.h) are exported and bound and fail cleanly without a
context; high_interest_mask restates src/CellFunctions.jl:42 and percentage_covered
src/FullSimulation.jl:557; Simulation's argument handling that needs no device."""
import ctypes
import math

import numpy as np
import pytest

REGION_SYMBOLS = ("mac_set_regions", "mac_regions_ingested", "mac_region_stats_f64")


def test_symbols_exported_and_bound(pkg):
    L = pkg.load_library()
    for s in REGION_SYMBOLS:
        assert s in pkg._lib.EXPORTS
        f = getattr(L, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int32
    assert pkg._lib.MAC_REGIONS_MAX == 64
    for m in ("set_regions", "clear_regions", "regions_ingested", "region_stats"):
        assert callable(getattr(pkg.Context, m))


def test_null_context_is_inval_and_writes_nothing(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int64)
    b = [np.array([v]) for v in (0.0, 1.0, 0.0, 1.0)]
    assert L.mac_set_regions(None, *(v.ctypes.data_as(dp) for v in b), 1, 5.0) == lib.MAC_E_INVAL
    assert "null" in L.mac_last_error().decode()
    assert L.mac_set_regions(None, None, None, None, None, 0, 5.0) == lib.MAC_E_INVAL
    bc = np.full(2, 7, dtype=np.int64)
    bw = np.full(2, 3.5)
    a, c = ctypes.c_int64(77), ctypes.c_int64(78)
    aw, cw = ctypes.c_double(-2.0), ctypes.c_double(-3.0)
    assert L.mac_regions_ingested(None, bc.ctypes.data_as(ip), ctypes.byref(a)) == lib.MAC_E_INVAL
    circ = np.array([0.0, 0.0, 1.0])
    assert L.mac_region_stats_f64(None, circ.ctypes.data_as(dp), 3, bc.ctypes.data_as(ip),
                                  bw.ctypes.data_as(dp), ctypes.byref(a), ctypes.byref(aw),
                                  ctypes.byref(c), ctypes.byref(cw)) == lib.MAC_E_INVAL
    assert np.all(bc == 7) and np.all(bw == 3.5)
    assert (a.value, c.value, aw.value, cw.value) == (77, 78, -2.0, -3.0)


# literal restatement of src/CellFunctions.jl:42 (1-based indices kept; the broadcast `.<` over the
# bound vectors and any(check))
def ref_check(new_point, x_LB, x_UB, y_LB, y_UB):
    p = [None] + list(new_point)
    check = [p[1] < x_UB[b] and p[1] > x_LB[b] and p[2] < y_UB[b] and p[2] > y_LB[b]
             for b in range(len(x_LB))]
    return any(check)


def test_high_interest_mask_matches_the_reference_loop(pkg):
    boxes = ([2500.0, 10.0, 5.0], [3500.0, 20.0, 5.0], [1000.0, -5.0, 0.0], [2000.0, 5.0, 9.0])
    xs, ys = [], []
    for xl, xu, yl, yu in zip(*boxes):   # on and one ulp beside every edge, and the corners
        ex = [v for e in (xl, xu) for v in (e, math.nextafter(e, -math.inf), math.nextafter(e, math.inf))]
        ey = [v for e in (yl, yu) for v in (e, math.nextafter(e, -math.inf), math.nextafter(e, math.inf))]
        for x in ex + [(xl + xu) / 2, math.nan, math.inf, -math.inf]:
            for y in ey + [(yl + yu) / 2, math.nan, math.inf, -math.inf]:
                xs.append(x)
                ys.append(y)
    xs, ys = np.array(xs), np.array(ys)
    got = pkg._lib.high_interest_mask(xs, ys, boxes)
    want = np.array([ref_check((x, y), *boxes) for x, y in zip(xs, ys)])
    assert got.dtype == bool and np.array_equal(got, want)
    assert want.any() and not want.all()
    # scalars (CellFunctions._high_interest's use), and the host mirror's override through it
    assert bool(pkg._lib.high_interest_mask(3000.0, 1500.0, boxes)) is True
    assert bool(pkg._lib.high_interest_mask(2500.0, 1500.0, boxes)) is False
    CF = pkg.CellFunctions
    w_hi = (30.0 * math.tan(100 / 180 * math.pi / 2)) ** 2 * math.pi
    p = CF._high_interest(np.array([3000.0, 1500.0, 25.0, 25.0, 0.0]), boxes, 30.0, 100 / 180 * math.pi)
    assert p[3] == w_hi and p[2] == 25.0
    p = CF._high_interest(np.array([3500.0, 1500.0, 25.0, 25.0, 0.0]), boxes, 30.0, 100 / 180 * math.pi)
    assert p[3] == 25.0


def test_percentage_formula(pkg):
    pc = pkg._lib.percentage_covered
    assert pc(0, 8) == 100.0
    assert pc(8, 8) == 0.0
    assert pc(3, 8) == 100 - (3 / 8) * 100
    assert pc(1, 3) == 100 - (1 / 3) * 100
    with np.errstate(all="raise"):   # total = 0: Julia's 0/0 = NaN, no exception and no warning
        assert math.isnan(pc(0, 0))


def test_simulation_arguments_without_a_device(pkg):
    FS = pkg.FullSimulation
    S = FS.Simulation
    assert S._boxes(None) is None
    assert S._boxes(True) == ([2500], [3500], [1000], [2000])
    assert S._boxes(([1], [2], [3], [4])) == ([1.0], [2.0], [3.0], [4.0])
    assert S._boxes((1, 2, 3, 4)) == ([1.0], [2.0], [3.0], [4.0])
    assert S._boxes(([1, 5], [2, 6], [3, 7], [4, 8])) == ([1.0, 5.0], [2.0, 6.0], [3.0, 7.0], [4.0, 8.0])
    for bad in (([1], [2], [3]), ([1, 2], [2], [3], [4]), ([], [], [], [])):
        with pytest.raises(ValueError):
            S._boxes(bad)
    with pytest.raises(ValueError):   # raised before the context is touched
        S(None, np.zeros(3), initial_points=np.zeros((0, 5)), w_high=100.0)
    # the r_max rule reads the boxes it is given; the module's stay the default
    t2 = math.tan(FS.FOV / 2)
    locs = np.array([3000.0, 100.0, 1500.0, 100.0, 15 * t2, 15 * t2])
    r = np.zeros(2)
    FS.r_max_update(locs, r, 2)
    assert r[0] == 15 * t2 and r[1] == FS.h_max * t2
    r = np.zeros(2)
    FS.r_max_update(locs, r, 2, ([90.0], [110.0], [90.0], [110.0]))
    assert r[0] == FS.h_max * t2 and r[1] == 15 * t2
