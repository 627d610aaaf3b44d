"""CPU: the progressive constraints' C-ABI and Python surface without a GPU (include/maxcover.h
mac_prog, mac_prog_h_f64, mac_mads_run_prog): struct sizes, every mac_prog error (checked before the
context is touched, so a NULL context reaches them), the Python ValueErrors and merge_mac_prog's
forms."""
import ctypes
import functools
import math

import numpy as np
import pytest


def _prog(lib, member, limit, n_cons, reserved=0, h_max0=-1.0):
    p = lib.make_prog(dict(member=member, limit=limit, n_cons=n_cons, h_max0=h_max0))
    p.reserved = reserved
    return p


def test_struct_sizes(pkg):
    lib = pkg._lib
    assert ctypes.sizeof(lib.Prog) == 32 and ctypes.sizeof(lib.MadsProgStats) == 80
    assert lib.Prog.h_max0.offset == 24 and lib.Prog.n_cons.offset == 16
    assert lib.MadsProgStats.f_feasible.offset == 8 and lib.MadsProgStats.evaluated.offset == 72
    assert {"mac_prog_h_f64", "mac_mads_run_prog"} <= set(lib.EXPORTS)
    assert lib.PROF_ROLES[10:] == ("prog_h_kernel", "prog_select_kernel")


def _h_call(pkg, prog, N=3, K=2):
    lib = pkg._lib
    L = pkg.load_library()
    X = np.zeros((K, 3 * N))
    out = np.full(K, 7.0)
    rc = L.mac_prog_h_f64(None, lib._ptr(X), 3 * N, K, ctypes.byref(prog) if prog is not None else None,
                          lib._ptr(out))
    return rc, L.mac_last_error().decode(), out


def test_mac_prog_errors_before_the_context(pkg):
    lib = pkg._lib
    ones, lim = np.ones(3, dtype=np.uint32), np.full(3, 35.0)
    bad = [
        _prog(lib, ones, lim, -1), _prog(lib, ones, lim, 33),          # n_cons outside [0, 32]
        _prog(lib, None, lim, 1), _prog(lib, ones, None, 1),           # n_cons > 0 with a null array
        _prog(lib, np.array([1, 2, 1], dtype=np.uint32), lim, 1),      # a bit at or above n_cons
        _prog(lib, np.array([1, 1, 1 << 31], dtype=np.uint32), lim, 31),
        _prog(lib, ones, lim, 1, reserved=1),                          # reserved
        _prog(lib, ones, np.array([35.0, math.nan, 35.0]), 1),         # a NaN limit
    ]
    for p in bad:
        rc, msg, out = _h_call(pkg, p)
        assert rc == lib.MAC_E_INVAL and "mac_prog" in msg, msg
        assert np.all(out == 7.0)                                      # nothing written
    big = _prog(lib, np.ones(2049, dtype=np.uint32), np.zeros(2049), 1)
    rc, msg, _ = _h_call(pkg, big, N=2049, K=1)
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "2048" in msg
    # a valid descriptor (32 constraints, the top bit used) gets as far as the context check
    ok = _prog(lib, np.array([1 << 31, 0, 0xFFFFFFFF], dtype=np.uint32), lim, 32)
    rc, msg, _ = _h_call(pkg, ok)
    assert rc == lib.MAC_E_INVAL and "null context" in msg
    rc, msg, _ = _h_call(pkg, _prog(lib, None, None, 0))
    assert rc == lib.MAC_E_INVAL and "null context" in msg


def _run_call(pkg, x0, prog):
    lib = pkg._lib
    L = pkg.load_library()
    x = np.asarray(x0, dtype=np.float64)
    N = x.size // 3
    rm = np.full(N, 35.0)
    out, xi = np.full_like(x, 7.0), np.full_like(x, 7.0)
    prm = lib.MadsParams(5, 2, 5, 99)
    st, ps = lib.MadsStats(), lib.MadsProgStats()
    ps.evaluated = -5
    rc = L.mac_mads_run_prog(None, lib._ptr(x), x.size, lib._ptr(rm), 0.0, None, None, 1.0, ctypes.byref(prm),
                             lib._ptr(out), ctypes.byref(st), None, None, None, None, ctypes.byref(prog),
                             lib._ptr(xi), ctypes.byref(ps))
    assert np.all(out == 7.0) and np.all(xi == 7.0) and ps.evaluated == -5   # nothing written
    return rc, L.mac_last_error().decode()


def test_mads_run_prog_start_errors_before_the_context(pkg):
    lib = pkg._lib
    ones, lim = np.ones(3, dtype=np.uint32), np.full(3, 35.0)
    x0 = np.array([1.0, 2, 3, 4, 5, 6, 36.0, 36.0, 34.0])
    nan0 = x0.copy()
    nan0[6] = math.nan
    rc, msg = _run_call(pkg, nan0, _prog(lib, ones, lim, 1))
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "NaN" in msg
    # h(x0) = (1 + 1)^2 = 4 > h_max0 = 3.5
    rc, msg = _run_call(pkg, x0, _prog(lib, ones, lim, 1, h_max0=3.5))
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "h_max0" in msg
    for p in (_prog(lib, ones, lim, 33), _prog(lib, ones, lim, 1, reserved=2),
              _prog(lib, np.array([1, 1, 2], dtype=np.uint32), lim, 1)):
        rc, msg = _run_call(pkg, x0, p)
        assert rc == lib.MAC_E_INVAL and "mac_prog" in msg
    # h_max0 = 4 admits x0, a negative or NaN h_max0 is the default: these reach the context check
    for h in (4.0, math.inf, -1.0, math.nan):
        rc, msg = _run_call(pkg, x0, _prog(lib, ones, lim, 1, h_max0=h))
        assert rc == lib.MAC_E_INVAL and "mac_prog" not in msg, msg


def test_python_value_errors(pkg):
    FS, TC = pkg.FullSimulation, pkg.TDM_Constraints
    x0 = np.array([1.0, 2, 3, 4, 5, 6, 36.0, 36.0, 34.0])
    prog = dict(member=np.ones(3, dtype=np.uint32), limit=np.full(3, 35.0), n_cons=1)
    with pytest.raises(ValueError, match="prog"):
        pkg.Context.mads_stepper(None, x0, np.full(3, 35.0), prog=prog)
    with pytest.raises(ValueError, match="cons_prog"):     # a callable without device data
        FS.Simulation(None, x0, initial_points=np.zeros((0, 5)), cons_prog=[lambda x: 0.0])
    with pytest.raises(ValueError, match="cons_prog"):     # a shard of more than one rank
        FS.Simulation(None, x0, initial_points=np.zeros((0, 5)), cons_prog=[TC.create_cons1_progressive],
                      shard=(0, 2), gather=object(), speculate=False)
    with pytest.raises(ValueError):
        TC.create_cons_progressive(-1, np.zeros(3))
    with pytest.raises(ValueError, match="member and limit"):
        pkg._lib.make_prog(dict(member=np.ones(2, dtype=np.uint32), limit=np.zeros(3), n_cons=1))


def test_merge_mac_prog_forms(pkg):
    TC = pkg.TDM_Constraints
    r_max = np.array([35.0, 36.0, 37.0, 38.0])
    mp, plain = TC.merge_mac_prog([TC.create_cons1_progressive(r_max)])
    assert not plain and mp["n_cons"] == 1
    assert mp["member"].dtype == np.uint32 and mp["member"].tolist() == [1, 1, 1, 1]
    assert mp["limit"].tolist() == r_max.tolist() and mp["limit"] is not r_max
    mp, plain = TC.merge_mac_prog([TC.create_cons_progressive(1, r_max), TC.create_cons_progressive(2, r_max)])
    assert not plain and mp["n_cons"] == 2 and mp["member"].tolist() == [0, 1, 2, 0]
    part = functools.partial(TC.create_cons_progressive, 3)
    mp, plain = TC.merge_mac_prog([TC.create_cons1_progressive(r_max), part(r_max)])
    assert mp["member"].tolist() == [1, 1, 1, 3] and mp["n_cons"] == 2
    # the limits are read when merging, as the callables read them when called
    r_max[0] = 30.0
    assert TC.merge_mac_prog([TC.create_cons1_progressive(r_max)])[0]["limit"][0] == 30.0
    plain_c = lambda x: 0.0   # noqa: E731
    other = TC.create_cons1_progressive(r_max + 1.0)
    mp, plain = TC.merge_mac_prog([TC.create_cons1_progressive(r_max), plain_c, other])
    assert mp["n_cons"] == 1 and plain == [plain_c, other]
    assert TC.merge_mac_prog([plain_c]) == (None, [plain_c]) and TC.merge_mac_prog([]) == (None, [])
    many = [TC.create_cons_progressive(0, r_max) for _ in range(33)]
    mp, plain = TC.merge_mac_prog(many)
    assert mp["n_cons"] == 32 and mp["member"][0] == 0xFFFFFFFF and len(plain) == 1
    # the callables: c(x) is the altitude excess, read against r_max at call time
    x = np.concatenate([np.zeros(8), [31.0, 36.5, 37.0, 40.0]])
    assert TC.create_cons1_progressive(r_max)(x) == ((0.0 + 1.0) + 0.5) + 0.0 + 2.0
    assert TC.create_cons_progressive(3, r_max)(x) == 2.0 and TC.create_cons_progressive(2, r_max)(x) == 0.0
