"""CPU: the swarm-constraint entry points (mac_cons, include/maxcover.h) are exported and bound,
fail cleanly without a context, and the host constraints create_cons8 / create_cons7 restate
src/TDM_Constraints.jl:142-172 and drive mads() to the same iterates as plain callables."""
import ctypes
import math

import numpy as np

CONS_SYMBOLS = ("mac_cons_mask_f64", "mac_cons_mask_dev_f64", "mac_poll_best_cons_f64",
                "mac_poll_best_cons_dev_f64")


def test_symbols_exported_and_bound(pkg):
    L = pkg.load_library()
    for s in CONS_SYMBOLS:
        assert s in pkg._lib.EXPORTS
        f = getattr(L, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int32
        assert ctypes.POINTER(pkg._lib.Cons) in f.argtypes


def test_mac_cons_layout(pkg):
    C = pkg._lib.Cons
    assert ctypes.sizeof(C) == 24
    assert [n for n, _ in C._fields_] == ["d_sep", "zone_y", "zone_r"]
    assert (C.d_sep.offset, C.zone_y.offset, C.zone_r.offset) == (0, 8, 16)
    assert pkg._lib.make_cons(None) is None
    c = pkg._lib.make_cons({"d_sep": 15.0})
    assert c.d_sep == 15.0 and math.isnan(c.zone_y) and math.isnan(c.zone_r)


def test_null_context_is_inval_and_writes_nothing(pkg):
    L = pkg.load_library()
    lib = pkg._lib
    cons = lib.Cons(15.0, float("nan"), float("nan"))
    cands = np.zeros((2, 6))
    p = cands.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.full(2, 7, dtype=np.uint8)
    op = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.mac_cons_mask_f64(None, p, 6, 2, ctypes.byref(cons), op) == lib.MAC_E_INVAL
    assert "null" in L.mac_last_error().decode()
    assert L.mac_cons_mask_dev_f64(None, None, 6, 2, ctypes.byref(cons), None, None) == lib.MAC_E_INVAL
    assert np.all(out == 7)
    rm = np.ones(2)
    objs = np.full(2, 3.5)
    bo, bi = ctypes.c_double(-2.0), ctypes.c_int64(77)
    dp = ctypes.POINTER(ctypes.c_double)
    for cp in (ctypes.byref(cons), None):   # a constraint on, and the forward to the plain call
        rc = L.mac_poll_best_cons_f64(None, p, 6, 2, rm.ctypes.data_as(dp), 1e5, None, None, 1.0,
                                      objs.ctypes.data_as(dp), ctypes.byref(bo), ctypes.byref(bi), cp)
        assert rc == lib.MAC_E_INVAL
        rc = L.mac_poll_best_cons_dev_f64(None, None, 6, 2, None, 1e5, None, None, 1.0, 0, None, None,
                                          None, cp)
        assert rc == lib.MAC_E_INVAL
    assert bo.value == -2.0 and bi.value == 77 and np.all(objs == 3.5)


# literal restatements of src/TDM_Constraints.jl:142-154 and :157-172 (1-based loops kept)
def ref_cons7(x, N, FOV):
    for i in range(1, N + 1):
        if x[i + N - 1] < 200:
            if x[i + 2 * N - 1] > 19 * math.tan(FOV / 2):
                return False
    return True


def ref_cons8(x, N):
    for i in range(1, N + 1):
        for j in range(1, N + 1):
            if j != i:
                hor_separation = math.sqrt((x[i - 1] - x[j - 1]) ** 2 + (x[i + N - 1] - x[j + N - 1]) ** 2)
                if hor_separation < 15.0:
                    return False
    return True


def test_create_cons8_matches_the_reference_loop(pkg):
    c8 = pkg.TDM_Constraints.create_cons8()
    assert c8.mac_cons == {"d_sep": 15.0}
    cases = [
        [0.0, 9.0, 0.0, 12.0, 5.0, 5.0],                       # exactly 15 apart: feasible
        [0.0, 9.0, 0.0, math.nextafter(12.0, 0.0), 5.0, 5.0],  # a hair closer: infeasible
        [1.0, 1.0, 2.0, 2.0, 5.0, 5.0],                        # coincident
        [3.0, 4.0, 6.0],                                       # N = 1
        [0.0, 100.0, 200.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0],
        [0.0, 100.0, 110.0, 0.0, 0.0, 5.0, 1.0, 1.0, 1.0],     # the last two 11.2 apart
    ]
    want = [True, False, False, True, True, False]
    for x, w in zip(cases, want):
        N = len(x) // 3
        assert ref_cons8(x, N) is w
        assert c8(np.array(x)) is w
    c20 = pkg.TDM_Constraints.create_cons8(20.0)
    assert c20.mac_cons == {"d_sep": 20.0}
    assert c20(np.array(cases[0])) is False


def test_create_cons7_matches_the_reference_loop(pkg):
    FOV = 100 / 180 * math.pi
    c7 = pkg.TDM_Constraints.create_cons7(FOV)
    r_lim = 19 * math.tan(FOV / 2)
    assert c7.mac_cons == {"zone_y": 200.0, "zone_r": r_lim}
    up = math.nextafter(r_lim, math.inf)
    cases = [
        ([0.0, 0.0, 100.0, 300.0, up, up], False),        # UAV 1 inside the zone, too high
        ([0.0, 0.0, 200.0, 300.0, up, up], True),         # y == 200 is outside the zone (strict <)
        ([0.0, 0.0, 100.0, 100.0, r_lim, r_lim], True),   # r == the cap is allowed (strict >)
        ([0.0, 0.0, 300.0, 199.0, 1.0, up], False),       # the last UAV
    ]
    for x, w in cases:
        assert ref_cons7(x, 2, FOV) is w
        assert c7(np.array(x)) is w


def test_merge_mac_cons(pkg):
    T = pkg.TDM_Constraints
    c8, c7 = T.create_cons8(), T.create_cons7(1.0)
    plain = lambda v: True   # noqa: E731
    merged, rest = T.merge_mac_cons([plain, c8, c7])
    assert merged == {"d_sep": 15.0, **c7.mac_cons} and rest == [plain]
    second = T.create_cons8(5.0)
    merged, rest = T.merge_mac_cons([c8, second])
    assert merged == {"d_sep": 15.0} and rest == [second]   # one slot: the second stays on the host
    assert T.merge_mac_cons([plain]) == (None, [plain])


def test_mads_iterates_do_not_depend_on_where_cons8_runs(pkg):
    """A stub batched objective (no GPU): mads() with cons8 as a plain host callable and with
    create_cons8 (handed to the poll as a mac_cons) visits the same incumbents."""
    target = np.array([40.0, 3.0, -35.0, 10.0, 44.0, -20.0, 5.0, 5.0, 5.0])
    c8 = pkg.TDM_Constraints.create_cons8(15.0)

    def plain_cons8(v):   # the same test without device data
        return c8(v)

    def make_obj(log):
        def obj(x):
            return float(np.sum((np.asarray(x) - target) ** 2))

        def poll(X, cons3=None, cons=None):
            o = np.array([obj(v) for v in X])
            if cons is not None:
                assert set(cons) == {"d_sep"}
                keep = np.array([pkg.TDM_Constraints.create_cons8(cons["d_sep"])(v) for v in X])
                o = np.where(keep, o, np.inf)
                log.append(int(np.count_nonzero(~keep)))
            k = int(np.argmin(o))
            obj.trace.append(float(o[k]))   # every poll's best objective: the iterates' record
            return (float(o[k]), k, o) if o[k] < np.inf else (np.inf, -1, o)

        obj.poll = poll
        obj.trace = []
        return obj

    x0 = np.array([0.0, 20.0, 40.0, 0.0, 0.0, 0.0, 5.0, 5.0, 5.0])
    log_dev, log_host = [], []
    oa, ob = make_obj(log_dev), make_obj(log_host)
    a = pkg.TDM_STATIC_opt.mads(x0, oa, [c8], N_iter=40, seed=11)
    b = pkg.TDM_STATIC_opt.mads(x0, ob, [plain_cons8], N_iter=40, seed=11)
    assert len(oa.trace) > 5 and oa.trace == ob.trace
    assert log_dev and sum(log_dev) > 0 and not log_host   # the device path took cons8 and it bit
    assert np.array_equal(a.x, b.x) and a.x_cost == b.x_cost
    assert a.status.iteration == b.status.iteration and a.status.successes == b.status.successes
    assert c8(a.x)
