"""The target-motion constraints cons4 / cons5 / cons6 (include/maxcover.h mac_motion) on the host:
the cone's acosd form against its threshold form, cons6's host-built thresholds against the direct
test, the data the callables carry for the device, and Simulation's derivation of the per-step arrays.
Needs no GPU (mac_motion_thresholds is host arithmetic)."""
import math

import numpy as np
import pytest

NAN = float("nan")
INF = float("inf")


def _ulps(v, k):
    """v and its k neighbours on either side (non-negative, finite)."""
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = math.nextafter(lo, -INF)
        hi = math.nextafter(hi, INF)
        out += [lo, hi]
    return [q for q in out if q >= 0.0 and q < INF]


def test_acosd_form_is_c_below_minus_half():
    """src/TDM_Constraints.jl:100: abs(acosd(round(c))) > 90 with Julia's round (ties to even, which
    np.round is)  <=>  c < -0.5, for c in [-1.25, 1.25] — c is a normalised dot product, within a few
    ulps of [-1, 1]; past +-1.5 round(c) leaves acosd's domain (Julia throws there) — and NaN."""
    cs = list(np.linspace(-1.25, 1.25, 20001))
    for v in (0.5, 1.0, 0.0, 0.25, 0.75, 1.25):
        for q in _ulps(v, 3):
            cs += [q, -q]
    cs += [NAN, -0.0]
    c = np.array(cs)
    with np.errstate(invalid="ignore"):
        acosd = np.degrees(np.arccos(np.round(c)))
        ref = np.abs(acosd) > 90
    assert np.array_equal(ref, c < -0.5)
    # the boundary itself: -0.5 rounds to -0 (90 degrees, feasible), its lower neighbour to -1
    assert np.round(-0.5) == 0 and not ref[cs.index(-0.5)]
    assert ref[cs.index(math.nextafter(-0.5, -INF))] and not ref[cs.index(math.nextafter(-0.5, INF))]
    assert not ref[-2]   # NaN: feasible


def _direct(q, p, a):
    return abs(math.sqrt(q) - p) > a


def test_cons6_thresholds_against_the_direct_form(pkg):
    """q3 > q_hi || q3 <= q_lo  <=>  |sqrt(q3) - p| > a for q3 within +-4 ulps of each threshold (and
    at 0, a few plain values and +inf), over (p, a) pairs including p < a, p = 0 and a = 0."""
    thr = pkg._lib.motion_thresholds
    rng = np.random.default_rng(11)
    pairs = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.5, 1.0), (1.0, 1.0), (2.0, 1.0), (3.0, 1.0),
             (1e-300, 1e-300), (1e16, 0.5), (1e-20, 1.0), (5e-324, 0.0), (1.0, 5e-324), (1e300, 1e300),
             (INF, 1.0), (1.0, INF), (-1.0, 0.5), (1.0, -1.0), (2.0, 2.0), (0.1, 0.3), (0.3, 0.1)]
    pairs += [(float(p), float(a)) for p, a in zip(rng.uniform(0, 4, 1500), rng.uniform(0, 2, 1500))]
    pairs += [(float(p), float(a)) for p, a in
              zip(10.0 ** rng.uniform(-12, 12, 1000), 10.0 ** rng.uniform(-12, 12, 1000))]
    pairs += [(float(np.round(p * 8) / 8), float(np.round(a * 8) / 8))      # exactly representable sums
              for p, a in zip(rng.uniform(0, 4, 500), rng.uniform(0, 2, 500))]
    assert len(pairs) > 3000
    sides = [0, 0]
    for p, a in pairs:
        hi, lo = thr(p, a)
        qs = [0.0, 1.0, 4.0, 1e-300, 1e300, INF]
        for T in (hi, lo):
            if 0.0 <= T < INF:
                qs += _ulps(T, 4)
        sides[0] += 0.0 <= hi < INF
        sides[1] += 0.0 <= lo < INF
        for q in qs:
            assert ((q > hi) or (q <= lo)) == _direct(q, p, a), (p, a, q, hi, lo)
    assert min(sides) > 500   # both sides have real thresholds in the sweep
    # NaN anywhere: every comparison false
    for p, a in ((NAN, 1.0), (1.0, NAN)):
        hi, lo = thr(p, a)
        assert hi == INF and lo == -1.0
    hi, lo = thr(1.0, 1.0)
    assert not (NAN > hi or NAN <= lo)


def test_cons5_threshold_is_cons3s(pkg):
    """cons5 on the device is q3 > dlim_threshold(v_max): the host callable against that form at the
    boundary (a 3-4-12 move of length 13, and v_max = 2 with q3 at 4 and its neighbours)."""
    TC = pkg.TDM_Constraints
    a = np.zeros(3)
    move = np.array([3.0, 4.0, 12.0])
    assert TC.create_cons5(a, 13.0)(move)                                  # 13 > 13 is false
    assert not TC.create_cons5(a, math.nextafter(13.0, -INF))(move)
    c5 = TC.create_cons5(a)
    assert c5.mac_motion["v_max"] == 2.0
    assert c5(np.array([2.0, 0.0, 0.0])) and not c5(np.array([math.nextafter(2.0, INF), 0.0, 0.0]))
    assert not c5(np.array([2.0, 0.0, 1e-3]))
    assert c5(np.array([NAN, 0.0, 0.0]))                                   # NaN: feasible


def test_cons4_host_callable(pkg):
    TC = pkg.TDM_Constraints
    a = np.zeros(3)
    c4 = TC.create_cons4([1.0, 0.0], a)
    assert c4.mac_motion["cone_cos"] == -0.5
    assert c4(np.array([5.0, 0.0, 7.0]))            # along the velocity
    assert c4(np.array([0.0, 5.0, 7.0]))            # 90 degrees
    assert not c4(np.array([-5.0, 0.0, 7.0]))       # straight back
    assert c4(np.array([-1.0, math.sqrt(3.0), 0.0])) == (TC.cone_cosine(1.0, 0.0, -1.0, math.sqrt(3.0)) >= -0.5)
    assert c4(np.array([0.0, 0.0, 9.0]))            # a zero move: c = NaN, feasible
    assert TC.create_cons4([0.0, 0.0], a)(np.array([-5.0, 0.0, 0.0]))   # a zero velocity
    assert math.isnan(TC.cone_cosine(0.0, 0.0, 1.0, 1.0)) and math.isnan(TC.cone_cosine(1.0, 0.0, INF, 0.0))
    assert TC.cone_cosine(2.0, 0.0, -1.0, 0.0) == -1.0 and TC.cone_cosine(0.0, 3.0, 4.0, 3.0) == 0.6


def test_split_cons_ext_returns_motion_data(pkg):
    TC, FS = pkg.TDM_Constraints, pkg.FullSimulation
    anchor = np.arange(6.0)
    m = FS.split_cons_ext([TC.create_cons5(anchor)])
    assert set(m) == {"motion"} and m["motion"]["v_max"] == 2.0
    assert np.array_equal(m["motion"]["anchor"], anchor)
    c4 = TC.create_cons4([1.0, 2.0, 3.0, 4.0], anchor)
    c6 = TC.create_cons6(anchor, [0.5, 1.5])
    m = FS.split_cons_ext([TC.cons1, TC.create_cons8(15.0), c4, TC.create_cons5(anchor), c6])
    assert m["d_sep"] == 15.0
    mo = m["motion"]
    assert (mo["cone_cos"], mo["v_max"], mo["a_max"]) == (-0.5, 2.0, 1.0)
    assert mo["vel"].tolist() == [1.0, 2.0, 3.0, 4.0] and mo["speed_prev"].tolist() == [0.5, 1.5]
    s = pkg._lib.make_motion(mo)
    assert (s.cone_cos, s.v_max, s.a_max, s.n_uav) == (-0.5, 2.0, 1.0, 2)
    assert [s.anchor[i] for i in range(6)] == anchor.tolist() and s.speed_prev[1] == 1.5
    off = pkg._lib.make_motion({"anchor": anchor})
    assert math.isnan(off.cone_cos) and math.isnan(off.v_max) and math.isnan(off.a_max) and not off.vel
    assert pkg._lib.make_motion(None) is None
    with pytest.raises(ValueError, match="cons5"):          # two of one kind: one slot
        FS.split_cons_ext([TC.create_cons5(anchor), TC.create_cons5(anchor, 3.0)])
    with pytest.raises(ValueError, match="cons6"):          # another anchor: one anchor
        FS.split_cons_ext([TC.create_cons5(anchor), TC.create_cons6(anchor + 1.0, [0.5, 1.5])])
    # merge_mac_cons / mads see them as device data as well
    merged, plain = TC.merge_mac_motion([c4, c6, TC.create_cons8(1.0)])
    assert set(merged) == {"anchor", "vel", "cone_cos", "speed_prev", "a_max"} and len(plain) == 1


def test_simulation_derives_the_motion_arrays(pkg):
    """anchor, vel and speed_prev on a hand-written three-step history (N = 2)."""
    FS = pkg.FullSimulation
    o1 = np.array([0.0, 10.0, 0.0, 10.0, 5.0, 5.0])
    o2 = np.array([3.0, 10.0, 4.0, 12.0, 5.0, 6.0])
    o3 = np.array([4.0, 8.0, 4.0, 9.0, 7.0, 12.0])
    prm = dict(cone_cos=-0.5, v_max=2.0, a_max=1.0)
    assert FS.derive_motion([], prm) is None and FS.derive_motion([o1], prm) is None
    m = FS.derive_motion([o1, o2], prm)
    assert np.array_equal(m["anchor"], o2)
    assert m["vel"].tolist() == [3.0, 0.0, 4.0, 2.0]
    assert m["speed_prev"].tolist() == [5.0, math.sqrt(5.0)]   # the moves (3, 4, 0) and (0, 2, 1)
    m = FS.derive_motion([o1, o2, o3], prm)
    assert np.array_equal(m["anchor"], o3)
    assert m["vel"].tolist() == [1.0, -2.0, 0.0, -3.0]
    assert m["speed_prev"].tolist() == [math.sqrt(1.0 + 0.0 + 4.0), 7.0]   # (1, 0, 2) and (-2, -3, 6)
    assert (m["cone_cos"], m["v_max"], m["a_max"]) == (-0.5, 2.0, 1.0)
    # a measured velocity instead of the last move; a constraint left out is off
    m = FS.derive_motion([o1, o2, o3], dict(cone_cos=-0.5), velocities=lambda t: [t, 0.0, 0.0, 1.0], t=4)
    assert m["vel"].tolist() == [4.0, 0.0, 0.0, 1.0] and "v_max" not in m and "speed_prev" not in m
    assert FS.derive_motion([o1, o2], {}) is None
    only5 = FS.derive_motion([o1, o2], dict(v_max=2.0))
    assert set(only5) == {"anchor", "v_max"}
    with pytest.raises(ValueError, match="cone_cos, v_max and a_max"):
        FS.Simulation(None, np.zeros(6), initial_points=np.zeros((0, 5)), motion=dict(vmax=2.0))
