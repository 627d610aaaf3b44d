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


# ---------------------------------------------------------------- steps 3-7 alone (prog_select_kernel's cases)

def _reference_record(pkg, case):
    """TDM_STATIC_opt.prog_select on a case, its tuple mapped to ProgRec's eight fields. The count is
    the arrays' own (prog_select takes the evaluated points and counts nothing); the best feasible
    candidate that does not improve comes from a second call without an F, which returns it."""
    TS = pkg.TDM_STATIC_opt
    K = case["K"]
    cands, evaluated = [], 0
    for c in (0, 1):
        if case["obj"][c] is None:
            continue
        f, h = case["obj"][c], case["h"][c]
        evaluated += int(np.count_nonzero(f != math.inf))
        cands += [(float(f[k]), float(h[k]), c, int(k)) for k in np.flatnonzero(f != math.inf)]
    F_f, I_f, I_h, h_max = pc.rule_args(case)
    outcome, bestF, newI, h_new = TS.prog_select(F_f, I_f, I_h, h_max, cands)
    any_F = TS.prog_select(None, I_f, I_h, h_max, cands)[1]
    assert bestF is None or bestF == any_F
    code = {"dominating": 0, "improving": 1, "unsuccessful": 2}[outcome] | (pc.REPLACES_F if bestF is not None else 0)
    bf = (math.inf, -1) if any_F is None else (any_F[0], any_F[1] * K + any_F[2])
    if newI is None:
        ni = (math.inf, math.inf, pc.NEW_I_NONE)
    elif newI == "old":
        ni = (I_f, I_h, pc.NEW_I_OLD)
    else:
        ni = (newI[0], newI[1], newI[2] * K + newI[3])
    return (code, bf[0], bf[1], ni[0], ni[1], ni[2], h_new, evaluated)


def _reference_records(pkg):
    if "select" not in _cache:
        _cache["select"] = [_reference_record(pkg, c) for c in pc.select_cases()]
    return _cache["select"]


def test_select_written_out_against_prog_select(pkg):
    """Every case of prog_cases.select_cases(): the rule written out one candidate at a time gives the
    record TDM_STATIC_opt.prog_select gives, field for field; a hand-written case also states it."""
    cases = pc.select_cases()
    assert cases is pc.select_cases() and len({c["name"] for c in cases}) == len(cases)
    hand = 0
    for case, ref in zip(cases, _reference_records(pkg)):
        got = pc.select_written_out(*pc.rule_args(case), case["obj"], case["h"], case["K"])
        assert pc.record_bytes(got) == pc.record_bytes(ref), (case["name"], got, ref)
        if case["want"] is not None:
            hand += 1
            assert pc.record_bytes(case["want"]) == pc.record_bytes(ref), (case["name"], case["want"], ref)
    assert hand >= 13


def test_select_cases_reach_every_class(pkg):
    """Counted on the reference's records alone: at least 20 cases of each outcome and of each kind
    of new I, every K x centres combination, every (has_F, has_I) but neither, and the edge values."""
    cases, recs = pc.select_cases(), _reference_records(pkg)
    n = dict(dom_F=0, dom_I=0, improving=0, unsuccessful=0, I_cand=0, I_old=0, I_none=0)
    for r in recs:
        kind = r[0] & 255
        n["dom_F"] += kind == 0 and bool(r[0] & pc.REPLACES_F)
        n["dom_I"] += kind == 0 and not r[0] & pc.REPLACES_F
        n["improving"] += kind == 1
        n["unsuccessful"] += kind == 2
        n["I_cand"] += r[5] >= 0
        n["I_old"] += r[5] == pc.NEW_I_OLD
        n["I_none"] += r[5] == pc.NEW_I_NONE
    assert all(v >= 20 for v in n.values()), n
    assert {(c["K"], c["centres"]) for c in cases} >= {(K, ce) for K in pc.SELECT_KS for ce in pc.CENTRES}
    assert {(c["has_F"], c["has_I"]) for c in cases} == {(1, 0), (0, 1), (1, 1)}
    assert any(c["has_I"] and c["I_f"] != c["I_f"] for c in cases) and any(c["F_f"] == math.inf for c in cases)
    # the unevaluated share: none, about half, all but one or two, all
    share = [r[7] / (c["K"] * (1 if c["centres"] != "both" else 2)) for c, r in zip(cases, recs)]
    assert any(s == 0.0 for s in share) and any(0.0 < s <= 2 / 63 for s in share)
    assert any(0.3 < s < 0.5 for s in share) and any(s > 0.7 for s in share)
    # the edge values occur among the evaluated candidates: NaN f, h = 5e-324, I.h's two neighbours
    seen = dict(nan=0, sub=0, below=0, above=0, at=0)
    for c in cases:
        for f, h in zip(c["obj"], c["h"]):
            if f is None or not c["has_I"]:
                continue
            ev = f != math.inf
            seen["nan"] += int(np.count_nonzero(f != f))
            seen["sub"] += int(np.count_nonzero(ev & (h == 5e-324)))
            seen["below"] += int(np.count_nonzero(ev & (h == np.nextafter(c["I_h"], -math.inf))))
            seen["above"] += int(np.count_nonzero(ev & (h == np.nextafter(c["I_h"], math.inf))))
            seen["at"] += int(np.count_nonzero(ev & (h == c["I_h"])))
    assert all(seen.values()), seen


def test_rowwise_cons3_is_create_cons3(pkg):
    """prog_cases.rowwise_cons3 (the larger-N runs' cons3) gives create_cons3's verdict: rows at,
    one ulp inside and one ulp outside the limit, in x, y and altitude, and random ones around it."""
    TC = pkg.TDM_Constraints
    N = 7
    rng = np.random.default_rng(3)
    x0 = np.concatenate([np.round(rng.uniform(100, 700, 2 * N)), np.full(N, 33.0)])
    c3 = TC.create_cons3(x0, pc.FOV, np.full(N, 10.0))
    fast = pc.rowwise_cons3(c3)
    rows = [x0.copy()]
    for v in range(3 * N):
        step = 10.0 * (pc.TAN50 if v >= 2 * N else 1.0)
        for d in (step, np.nextafter(step, 0.0), np.nextafter(step, 100.0), -step, 6.0, 8.0):
            r = x0.copy()
            r[v] += d
            rows.append(r)
    for i in range(N):   # (6, 8, 0) is at the limit exactly
        r = x0.copy()
        r[i] += 6.0
        r[N + i] += 8.0
        rows.append(r)
    rows += list(x0[None, :] + np.round(rng.uniform(-7.0, 7.0, (200, 3 * N))))
    got = [fast(r) for r in rows]
    assert got == [c3(r) for r in rows] and min(got.count(True), got.count(False)) >= 20
    assert fast.prev is c3.prev and fast.tan_half_fov == c3.tan_half_fov
