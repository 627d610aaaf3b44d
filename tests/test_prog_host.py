"""CPU: the progressive barrier on the host mirrors alone (DESIGN.md section 4 "Progressive
barrier"; src/TDM_Constraints.jl:182-220 handed to MADS at src/TDM_STATIC_opt.jl:142-159).
TDM_STATIC_opt.mads(cons_prog=) against the rule written out in tests/prog_cases.py one trial point
at a time, over the oracle's objective with penalty 0; the arithmetic of h; cons_prog=() is the
call without the keyword. Every comparison is exact."""
import math

import numpy as np
import pytest

import prog_cases as pc

_cache = {}


def _nan_eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _case(pkg, orc, radii, two, gran, poll_vars):
    key = (radii, two, gran, poll_vars)
    if key not in _cache:
        TS, TC, lib = pkg.TDM_STATIC_opt, pkg.TDM_Constraints, pkg._lib
        N = 3
        rec, x0, r_max = pc.recipe(pkg, N, 7, 320, 40, radii)
        obj = lambda v: orc.ref_objective(v, rec, r_max, 0.0)   # noqa: E731
        c3 = TC.create_cons3(x0, pc.FOV, np.full(N, 10.0))
        if two:   # the reference's cons2_progressive and cons3_progressive: UAVs 2 and 3
            progs = [TC.create_cons_progressive(1, r_max), TC.create_cons_progressive(2, r_max)]
            member, J = [0, 1, 2], 2
        else:
            progs = [TC.create_cons1_progressive(r_max)]
            member, J = [1, 1, 1], 1
        res = TS.mads(x0, obj, [TC.cons1, c3], cons_prog=progs, granularity=gran, poll_vars=poll_vars,
                      **pc.KW)
        g = lib.mesh_granularity(gran, x0.size)
        want = pc.rule_written_out(pkg, obj, [c3], member, r_max, J, x0, g,
                                   TS.polled_count(x0.size, poll_vars), **pc.KW)
        _cache[key] = res, want, x0
    return _cache[key]


@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
@pytest.mark.parametrize("gran", [None, (1.0, 0.125)])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("radii", [35.0, 36.0, 38.0])
def test_mads_cons_prog_against_the_written_out_rule(pkg, orc, radii, two, gran, poll_vars):
    res, want, x0 = _case(pkg, orc, radii, two, gran, poll_vars)
    s = res.status
    assert len(res.history) == len(want["iters"]) == s.iteration == want["it"]
    for got, ref in zip(res.history, want["iters"]):
        assert got[0] == ref[0] and got[7] == ref[7]
        assert _nan_eq(got[1], ref[1]) and got[2] == ref[2]          # F.x, F.f
        assert _nan_eq(got[3], ref[3]) and got[4] == ref[4] and got[5] == ref[5]   # I.x, I.f, I.h
        assert got[6] == ref[6]                                       # h_max
    F, I = want["F"], want["I"]
    assert _nan_eq(res.x, None if F is None else F[0]) and res.x_cost == (math.inf if F is None else F[1])
    assert _nan_eq(res.i, None if I is None else I[0])
    if I is not None:
        assert (res.i_cost, res.i_h) == (I[1], I[2])
    assert res.h_max == want["h_max"]
    assert (s.dominating, s.improving, s.unsuccessful) == \
        (want["dominating"], want["improving"], want["unsuccessful"])
    assert s.successes == want["dominating"]
    assert s.two_centre_polls == want["two"] and s.evaluated == want["evaluated"]
    assert s.function_evaluations == want["evals"]
    assert s.optimization_status == want["status"]
    if poll_vars == "xy":   # the radii are held: h never changes
        hs = {r[5] for r in want["iters"] if r[5] is not None}
        assert len(hs) <= 1 and want["improving"] == 0
        assert want["h_max"] == (hs.pop() if hs else math.inf)


@pytest.mark.parametrize("radii,two", [(36.0, False), (38.0, False), (38.0, True)])
def test_every_outcome_and_a_two_centre_poll_occur(pkg, orc, radii, two):
    """On the reference side (the written-out rule), so that no case above passes trivially."""
    want = _case(pkg, orc, radii, two, None, "xyr")[1]
    for k in ("dominating", "improving", "unsuccessful", "two"):
        assert want[k] >= 1, k


def test_h_arithmetic(pkg):
    TC = pkg.TDM_Constraints
    lim = np.array([35.75, 35.75, 35.75])
    up, down = np.nextafter(35.75, np.inf), np.nextafter(35.75, -np.inf)
    c1 = TC.create_cons1_progressive(lim)

    def h(radii, progs=(c1,)):
        x = np.concatenate([np.zeros(6), np.asarray(radii, dtype=np.float64)])
        return TC.prog_h([c(x) for c in progs])

    assert h([35.75, 35.75, 35.75]) == 0.0 and h([down, 1.0, -5.0]) == 0.0   # at or below the limit
    e = up - 35.75
    assert h([up, 35.75, 35.75]) == e * e > 0.0                               # one ulp above
    # c = 2^-600 exactly: its square underflows to 0.0, which counts as feasible
    tiny = TC.create_cons1_progressive(np.zeros(3))
    x = np.concatenate([np.zeros(6), [2.0 ** -600, 0.0, -1.0]])
    assert tiny(x) == 2.0 ** -600 and TC.prog_h([tiny(x)]) == 0.0
    # NaN R: Julia's max keeps it (Python's max and fmax would not)
    assert math.isnan(c1(np.concatenate([np.zeros(6), [math.nan, 36.0, 36.0]])))
    assert math.isnan(h([36.0, math.nan, 36.0])) and math.isnan(h([0.0, 0.0, math.nan]))
    assert TC.prog_term(math.nan, 1.0) != TC.prog_term(math.nan, 1.0) and max(0.0, math.nan) == 0.0
    # the fold's order over i: (1 + 2^-53) + 2^-53 = 1 in this order, 1 + 2^-52 in the other
    z = TC.create_cons1_progressive(np.zeros(3))
    u = 2.0 ** -53
    fwd = z(np.concatenate([np.zeros(6), [1.0, u, u]]))
    rev = z(np.concatenate([np.zeros(6), [u, u, 1.0]]))
    assert fwd == 1.0 and rev == 1.0 + 2.0 ** -52
    assert pc.h_written_out(np.concatenate([np.zeros(6), [1.0, u, u]]), [1, 1, 1], np.zeros(3), 1) == 1.0
    # ... and over j: h = ((c0^2 + c1^2) + c2^2)
    cs = [1.0, 1.25 * 2.0 ** -27, 1.25 * 2.0 ** -27]   # squares 1 and twice 0.39 ulp(1)
    assert TC.prog_h(cs) == 1.0 and TC.prog_h(cs[::-1]) == 1.0 + 2.0 ** -52
    # each product is rounded before its add (an FMA would keep 2^-60 here)
    c = 1.0 + 2.0 ** -30
    assert TC.prog_h([c]) == c * c and TC.prog_h([1.0, c]) == 1.0 + c * c


def test_a_nan_h_candidate_is_dropped_and_h_x0_nan_is_an_error(pkg, orc):
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max = pc.recipe(pkg, 3, 7, 320, 40, 36.0)
    obj = lambda v: orc.ref_objective(v, rec, r_max, 0.0)   # noqa: E731

    def nan_above_37(x):   # a plain callable: NaN for every trial point with a radius above 37
        return math.nan if np.any(np.asarray(x)[6:] > 37.0) else 0.0

    res = TS.mads(x0, obj, [], cons_prog=[nan_above_37], **pc.KW)
    assert res.x is not None and np.all(res.x[6:] <= 37.0) and res.i is None
    assert all(np.all(r[1][6:] <= 37.0) for r in res.history)
    assert res.status.evaluated < res.status.function_evaluations - 1   # some were dropped
    bad = x0.copy()
    bad[6] = math.nan
    with pytest.raises(ValueError, match="NaN"):
        TS.mads(bad, obj, [], cons_prog=[TC.create_cons1_progressive(r_max)], **pc.KW)
    with pytest.raises(ValueError, match="h_max0"):
        TS.mads(x0, obj, [], cons_prog=[TC.create_cons1_progressive(r_max)], h_max0=1e-3, **pc.KW)


def test_h_max0(pkg, orc):
    """A given h_max0 is the first threshold; negative or NaN means the default, h(x0)."""
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max = pc.recipe(pkg, 3, 7, 320, 40, 36.0)
    obj = lambda v: orc.ref_objective(v, rec, r_max, 0.0)   # noqa: E731
    progs = [TC.create_cons1_progressive(r_max)]
    base = TS.mads(x0, obj, [], cons_prog=progs, **pc.KW)
    for h0 in (-1.0, math.nan):
        res = TS.mads(x0, obj, [], cons_prog=progs, h_max0=h0, **pc.KW)
        assert _nan_eq(res.x, base.x) and res.h_max == base.h_max and \
            [r[0] for r in res.history] == [r[0] for r in base.history]
    wide = TS.mads(x0, obj, [], cons_prog=progs, h_max0=math.inf, **pc.KW)
    want = pc.rule_written_out(pkg, obj, [], [1, 1, 1], r_max, 1, x0, None, 9, h_max0=math.inf, **pc.KW)
    assert [r[0] for r in wide.history] == [r[0] for r in want["iters"]]
    assert _nan_eq(wide.x, want["F"][0] if want["F"] else None) and wide.h_max == want["h_max"]
    assert wide.status.evaluated == want["evaluated"] >= base.status.evaluated


def test_empty_cons_prog_is_the_call_without_the_keyword(pkg, orc):
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max = pc.recipe(pkg, 3, 7, 320, 40, 36.0)
    obj = lambda v: orc.ref_objective(v, rec, r_max, 1e5)   # noqa: E731
    c3 = TC.create_cons3(x0, pc.FOV, np.full(3, 10.0))
    a = TS.mads(x0, obj, [c3], **pc.KW)
    b = TS.mads(x0, obj, [c3], cons_prog=(), **pc.KW)
    c, _ = TS.optimize(x0, obj, [c3], [], pc.KW["N_iter"])
    d = TS.mads(x0, obj, [c3], pc.KW["N_iter"])
    assert a.x.tobytes() == b.x.tobytes() and a.x_cost == b.x_cost and b.history == []
    assert c.tobytes() == d.x.tobytes()
    for k in ("iteration", "function_evaluations", "cons3_passed", "cons3_empty_polls", "successes",
              "optimization_status", "dominating", "improving", "unsuccessful"):
        assert getattr(a.status, k) == getattr(b.status, k), k
    assert (b.status.dominating, b.status.improving, b.status.unsuccessful) == (0, 0, 0)


def test_optimize_passes_cons_prog_on(pkg, orc):
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max = pc.recipe(pkg, 3, 7, 320, 40, 36.0)
    obj = lambda v: orc.ref_objective(v, rec, r_max, 0.0)   # noqa: E731
    progs = [TC.create_cons1_progressive(r_max)]
    got, _ = TS.optimize(x0, obj, [], progs, 10)
    want = TS.mads(x0, obj, [], 10, cons_prog=progs)
    assert got.tobytes() == (want.x if want.x is not None else want.i).tobytes()
    plain = TS.mads(x0, obj, [], 10)
    assert got.tobytes() != plain.x.tobytes()   # (penalty 0: without the constraint the radii grow)
