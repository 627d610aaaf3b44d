"""CPU: TDM_Constraints.explain, the host mirror of mac_verdict (the documented meaning of the record),
against an O(N^2) brute force written here, and the identity "bit q <=> not create_consq(...)(x)" on
seeded trial points. Every comparison is exact: the record holds integers."""
import math

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")
FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)
KINDS = ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")


def brute(x, d_sep=NAN, zone=(NAN, NAN), prev=None, d_lim=None, t=TAN50, anchor=None, vel=None,
          speed_prev=None, cone_cos=NAN, v_max=NAN, a_max=NAN):
    """The record as a dict, straight from the constraints' definitions (src/TDM_Constraints.jl): plain
    Python floats, one UAV and one ordered pair at a time."""
    x = [float(v) for v in x]
    N = len(x) // 3
    bad = {k: set() for k in KINDS}
    pairs = 0
    sq = math.sqrt   # (nan -> nan, inf -> inf; the sums of squares here are never negative)
    for i in range(N):
        xi, yi, ri = x[i], x[N + i], x[2 * N + i]
        if prev is not None:
            dx, dy, dz = prev[i] - xi, prev[N + i] - yi, prev[2 * N + i] / t - ri / t
            if sq(dx * dx + dy * dy + dz * dz) > d_lim[i]:
                bad["cons3"].add(i)
        if zone[0] == zone[0] and zone[1] == zone[1] and yi < zone[0] and ri > zone[1]:
            bad["cons7"].add(i)
        if d_sep > 0.0:
            for j in range(N):
                if j == i:
                    continue
                dx, dy = xi - x[j], yi - x[N + j]
                if sq(dx * dx + dy * dy) < d_sep:
                    bad["cons8"].add(i)
                    pairs += j > i
        if anchor is not None:
            tx, ty, tz = xi - anchor[i], yi - anchor[N + i], ri - anchor[2 * N + i]
            q2 = tx * tx + ty * ty
            s3 = sq(q2 + tz * tz)
            if v_max == v_max and s3 > v_max:
                bad["cons5"].add(i)
            if a_max == a_max and speed_prev is not None and abs(s3 - speed_prev[i]) > a_max:
                bad["cons6"].add(i)
            if cone_cos == cone_cos and vel is not None:
                ux, uy = float(vel[i]), float(vel[N + i])
                den = sq(ux * ux + uy * uy) * sq(q2)
                num = ux * tx + uy * ty
                with np.errstate(all="ignore"):
                    c = float(np.float64(num) / np.float64(den))
                if c < cone_cos:
                    bad["cons4"].add(i)
    return dict(reasons=sum(1 << q for q, k in enumerate(KINDS) if bad[k]), pairs=pairs,
                n_uav=[len(bad[k]) for k in KINDS], first_uav=[min(bad[k]) if bad[k] else -1 for k in KINDS])


def as_dict(rec):
    assert rec.dtype.itemsize == 64 and rec["reserved"].tolist() == [0, 0]
    return dict(reasons=int(rec["reasons"]), pairs=int(rec["pairs"]), n_uav=rec["n_uav"].tolist(),
                first_uav=rec["first_uav"].tolist())


def _setup(pkg, N, seed):
    """Seeded integer data around a lattice: anchor = prev, moves of up to 3 per coordinate of two UAVs."""
    rng = np.random.default_rng(seed)
    side = max(1, int(math.ceil(math.sqrt(N))))
    ix, iy = np.divmod(np.arange(N), side)
    anchor = np.concatenate([100.0 + 6.0 * ix, 100.0 + 6.0 * iy, np.full(N, 12.0)])
    vel = np.concatenate([rng.integers(-2, 3, N), rng.integers(-2, 3, N)]).astype(np.float64)
    speed_prev = rng.integers(0, 2, N).astype(np.float64)   # (a UAV that stays passes cons6)
    d_lim = rng.integers(3, 7, N).astype(np.float64)
    xs = []
    for _ in range(16):   # two UAVs move per trial point, so that every kind lets some points through
        x = anchor.copy()
        for i in rng.choice(N, size=min(N, 2), replace=False):
            x[[i, N + i, 2 * N + i]] += rng.integers(-3, 4, 3).astype(np.float64)
        xs.append(x)
    return anchor, vel, speed_prev, d_lim, xs


@pytest.mark.parametrize("N", [1, 2, 7, 30])
def test_against_the_brute_force_and_the_callables(pkg, N):
    TC = pkg.TDM_Constraints
    anchor, vel, speed_prev, d_lim, xs = _setup(pkg, N, 100 + N)
    zone_y, h_above = 106.0, 12.0 / TAN50
    cs = [TC.create_cons3(anchor, FOV, d_lim), TC.create_cons8(5.0), TC.create_cons7(FOV, zone_y, h_above),
          TC.create_cons4(vel, anchor, -0.5), TC.create_cons5(anchor, 4.0), TC.create_cons6(anchor, speed_prev, 3.0)]
    zr = cs[2].mac_cons["zone_r"]
    seen = np.zeros(6, dtype=int)
    for x in xs:
        got = as_dict(TC.explain(x, cs))
        want = brute(x, 5.0, (zone_y, zr), anchor, d_lim, cs[0].tan_half_fov, anchor, vel, speed_prev, -0.5, 4.0, 3.0)
        assert got == want
        for q, c in enumerate(cs):   # the identity, kind by kind
            assert bool(got["reasons"] >> q & 1) == (not c(x)), (q, x)
            # ... and the kind alone gives the same bit, counts and index
            one = as_dict(TC.explain(x, [c]))
            assert one["reasons"] == got["reasons"] & (1 << q)
            assert one["n_uav"][q] == got["n_uav"][q] and one["first_uav"][q] == got["first_uav"][q]
        seen += [got["reasons"] >> q & 1 for q in range(6)]
        # the descriptor form and the raw cons3 arguments give the same record
        desc = dict(cons={"d_sep": 5.0, "zone_y": zone_y, "zone_r": zr},
                    motion={"anchor": anchor, "vel": vel, "speed_prev": speed_prev, "cone_cos": -0.5,
                            "v_max": 4.0, "a_max": 3.0})
        assert as_dict(TC.explain(x, desc, prev=anchor, d_lim=d_lim, FOV=FOV)) == got
    if N == 1:
        assert seen[1] == 0   # no pairs
    if N >= 7:   # both classes of every kind occur
        assert np.all(seen > 0) and np.all(seen < len(xs)), seen


def test_spacing_boundary(pkg):
    """The pair test is a strict <: exactly d_sep apart is feasible, one ulp inside is not."""
    TC = pkg.TDM_Constraints
    d = 15.0
    x = np.array([100.0, 115.0, 50.0, 50.0, 3.0, 3.0])
    assert as_dict(TC.explain(x, {"d_sep": d})) == brute(x, d) == dict(
        reasons=0, pairs=0, n_uav=[0] * 6, first_uav=[-1] * 6)
    x[1] = np.nextafter(115.0, 0.0)
    got = as_dict(TC.explain(x, {"d_sep": d}))
    assert got == brute(x, d)
    assert got == dict(reasons=2, pairs=1, n_uav=[0, 2, 0, 0, 0, 0], first_uav=[-1, 0, -1, -1, -1, -1])
    assert not TC.create_cons8(d)(x)


def test_coincident_and_non_finite(pkg):
    TC = pkg.TDM_Constraints
    N = 6
    x = np.concatenate([np.full(N, 7.0), np.full(N, -3.0), np.full(N, 2.0)])
    got = as_dict(TC.explain(x, [TC.create_cons8(1e-3)]))
    assert got == brute(x, 1e-3)
    assert got["pairs"] == N * (N - 1) // 2 and got["n_uav"][1] == N and got["first_uav"][1] == 0
    # a NaN or infinite coordinate: that UAV is in no pair, the others still are
    for badv in (NAN, INF, -INF):
        for slot in (2, N + 2):
            y = x.copy()
            y[slot] = badv
            got = as_dict(TC.explain(y, {"d_sep": 1e-3}))
            assert got == brute(y, 1e-3)
            assert got["pairs"] == (N - 1) * (N - 2) // 2 and got["n_uav"][1] == N - 1
    # NaN operands reject nothing under the per-UAV kinds either
    a = np.zeros(3)
    rec = TC.explain(np.array([NAN, NAN, NAN]), dict(zone_y=1.0, zone_r=0.0, anchor=a, vel=np.ones(2),
                                                     speed_prev=np.zeros(1), cone_cos=-0.5, v_max=1.0,
                                                     a_max=1.0), prev=a, d_lim=np.ones(1), FOV=FOV)
    assert int(rec["reasons"]) == 0 and rec["first_uav"].tolist() == [-1] * 6


def test_zero_velocity_and_zero_move(pkg):
    """cons4's cosine is 0/0 = NaN with a zero velocity or a zero move: feasible."""
    TC = pkg.TDM_Constraints
    a = np.array([10.0, 20.0, 30.0, 40.0, 5.0, 5.0])
    vel = np.array([0.0, 1.0, 0.0, 0.0])
    x = a + np.array([-3.0, 0.0, 0.0, 0.0, 0.0, 0.0])   # UAV 0 moves against nothing; UAV 1 stays
    c4 = TC.create_cons4(vel, a, -0.5)
    got = as_dict(TC.explain(x, [c4]))
    assert got == brute(x, anchor=a, vel=vel, cone_cos=-0.5) and got["reasons"] == 0 and c4(x)
    x[1] -= 2.0   # UAV 1 now moves straight against its velocity
    got = as_dict(TC.explain(x, [c4]))
    assert got["reasons"] == 8 and got["n_uav"][3] == 1 and got["first_uav"][3] == 1 and not c4(x)


def test_every_kind_off(pkg):
    TC = pkg.TDM_Constraints
    x = np.array([0.0, 0.0, 0.0, 0.0, 99.0, 99.0])
    none = dict(reasons=0, pairs=0, n_uav=[0] * 6, first_uav=[-1] * 6)
    a = np.zeros(6)
    for given in (None, [], {}, {"d_sep": 0.0}, {"d_sep": -1.0, "zone_y": 5.0}, {"d_sep": NAN, "zone_r": 1.0},
                  {"anchor": a, "cone_cos": -0.5, "a_max": 0.0},          # no vel, no speed_prev
                  {"anchor": a, "vel": np.ones(4), "speed_prev": np.zeros(2)},   # every scalar NaN
                  {"vel": np.ones(4), "cone_cos": -0.5, "v_max": 0.0},    # no anchor
                  [TC.cons1]):
        assert as_dict(TC.explain(x, given)) == none, given
    with pytest.raises(ValueError):
        TC.explain(x, None, prev=a)
