"""GPU: the target-motion constraints on the device (mac_motion: cons4 cone, cons5 speed, cons6
acceleration; k_cons.h motion_rejects) in the mask and the masked matrix poll, against the host
callables TDM_Constraints.create_cons4 / 5 / 6. Every comparison is exact equality.

The expected masks come from a numpy restatement (elementwise tx*tx + ty*ty, np.sqrt, /: numpy does
not fuse) that is itself compared with the host callables, candidate by candidate, at the small sizes
and on a sample of candidates at the large ones. The candidates carry, on the last UAV (anchor 0, so
its move is the coordinate itself): q3 exactly at cons5's threshold and at both neighbouring doubles,
the same on both sides of cons6, and the cone's c at -0.5 and at the doubles on either side; these
ladders are the check that the device's fp64 sqrt and division round correctly."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")
TAN50 = math.tan(100 / 180 * math.pi / 2)
PITCH = 13.0
V_MAX, A_MAX, CONE = 2.0, 1.0, -0.5        # the reference's values
P_LAST, U_LAST = 1.25, (1.0, 0.25)          # the ladder UAV's speed_prev and velocity


# ---------------------------------------------------------------- the yardstick

def yard(C, mo):
    """feasible[k] of the K x 3N matrix C per constraint: dict name -> bool[K] (only those on)."""
    C = np.asarray(C, dtype=np.float64)
    a = mo["anchor"]
    N = a.size // 3
    out = {}
    with np.errstate(all="ignore"):
        tx, ty, tz = C[:, :N] - a[:N], C[:, N:2 * N] - a[N:2 * N], C[:, 2 * N:] - a[2 * N:]
        q2 = tx * tx + ty * ty
        q3 = q2 + tz * tz
        if "v_max" in mo:
            out["cons5"] = ~np.any(np.sqrt(q3) > mo["v_max"], axis=1)
        if "a_max" in mo:
            out["cons6"] = ~np.any(np.abs(np.sqrt(q3) - mo["speed_prev"]) > mo["a_max"], axis=1)
        if "cone_cos" in mo:
            ux, uy = mo["vel"][:N], mo["vel"][N:]
            c = (ux * tx + uy * ty) / (np.sqrt(ux * ux + uy * uy) * np.sqrt(q2))
            out["cons4"] = ~np.any(c < mo["cone_cos"], axis=1)
    return out


def yard_cons8(C, a, d_sep):
    """cons8 over the pairs whose anchors are less than d_sep + 6 apart: no finite coordinate of C is
    3 or more from its anchor (asserted), so no other pair can come closer than d_sep; a pair with a
    non-finite coordinate is at distance inf or NaN, never < d_sep."""
    C = np.asarray(C, dtype=np.float64)
    N = C.shape[1] // 3
    if N < 2:
        return np.ones(C.shape[0], dtype=bool)
    dev = np.abs(C - a)
    assert np.all(dev[np.isfinite(dev)] < 3.0)
    ax, ay = a[:N], a[N:2 * N]
    near = np.hypot(ax[:, None] - ax[None, :], ay[:, None] - ay[None, :]) < d_sep + 6.0
    i, j = np.nonzero(np.triu(near, 1))
    with np.errstate(all="ignore"):
        dx, dy = C[:, i] - C[:, j], C[:, N + i] - C[:, N + j]
        return ~np.any(np.sqrt(dx * dx + dy * dy) < d_sep, axis=1)


def callables(pkg, mo):
    TC = pkg.TDM_Constraints
    out = {}
    if "v_max" in mo:
        out["cons5"] = TC.create_cons5(mo["anchor"], mo["v_max"])
    if "a_max" in mo:
        out["cons6"] = TC.create_cons6(mo["anchor"], mo["speed_prev"], mo["a_max"])
    if "cone_cos" in mo:
        out["cons4"] = TC.create_cons4(mo["vel"], mo["anchor"], mo["cone_cos"])
    return out


# ---------------------------------------------------------------- data

def _q3(t):
    return (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]


def move_with_q3(q):
    """(tx, ty, tz), all > 0, with fl(fl(fl(tx*tx) + fl(ty*ty)) + fl(tz*tz)) == q exactly: tx and ty are
    fp32 values (their squares and the sum of the squares are exact doubles), tz the root of what
    is left, whose rounding is far below q's half ulp."""
    tx = float(np.float32(0.9 * math.sqrt(q)))
    ty = float(np.float32(math.sqrt(0.9 * (q - tx * tx))))
    tz = math.sqrt(q - (tx * tx + ty * ty))
    t = (tx, ty, tz)
    assert _q3(t) == q, (q, t)
    return t


def cone_ladder(pkg):
    """Moves (tx, ty) of the ladder UAV (velocity U_LAST) whose c is exactly -0.5, the double below
    and the double above: a host search over the ulps of ty around the 120-degree direction."""
    cc = pkg.TDM_Constraints.cone_cosine
    want = {CONE: None, math.nextafter(CONE, -INF): None, math.nextafter(CONE, INF): None}
    th = math.atan2(U_LAST[1], U_LAST[0]) + 2.0 * math.pi / 3.0
    rng = np.random.default_rng(4)
    for _ in range(400):
        r = float(rng.uniform(0.4, 1.2))
        tx, ty = r * math.cos(th), r * math.sin(th)
        for _ in range(48):
            ty = math.nextafter(ty, -INF)
        for _ in range(96):
            ty = math.nextafter(ty, INF)
            c = cc(U_LAST[0], U_LAST[1], tx, ty)
            if c in want and want[c] is None:
                want[c] = (tx, ty)
        if all(v is not None for v in want.values()):
            break
    assert all(v is not None for v in want.values()), want
    return [want[k] for k in sorted(want)]   # below (rejected), at -0.5, above


_DATA = {}


def build(pkg, N, K=70):
    """(C, motion mapping): anchors on a lattice of pitch 13 with the last UAV at the origin (radius
    0: its move is its coordinate), UAV 0 pulled to 10.4 from UAV 1 and given a zero velocity."""
    if (N, K) in _DATA:
        return _DATA[(N, K)]
    rng = np.random.default_rng(1000 + N)
    side = max(2, math.ceil(math.sqrt(N)))
    ix, iy = np.divmod(np.arange(N), side)
    ax, ay = PITCH * (ix - ix[-1]), PITCH * (iy - iy[-1])
    ar = np.full(N, 6.0)
    ar[-1] = 0.0
    if N >= 2:
        ay[0] += 2.6
    a = np.concatenate([ax, ay, ar]).astype(np.float64)
    ang = rng.uniform(0, 2 * math.pi, N)
    sp = rng.uniform(0.5, 2.0, N)
    ux, uy = sp * np.cos(ang), sp * np.sin(ang)
    p = rng.uniform(1.05, 1.5, N)
    ux[-1], uy[-1], p[-1] = U_LAST[0], U_LAST[1], P_LAST
    if N >= 2:
        ux[0] = uy[0] = 0.0                       # a zero velocity: c = NaN, cons4 never rejects UAV 0
    if N >= 3:
        ux[1], uy[1] = 0.0, -1.0                  # UAV 1 heads for UAV 0, 10.4 away
    mo = dict(anchor=a, vel=np.concatenate([ux, uy]), speed_prev=p, cone_cos=CONE, v_max=V_MAX, a_max=A_MAX)
    uang = np.arctan2(uy, ux)

    def base():
        """Every UAV moves by p - 0.9 .. p - 0.5 within 50 degrees of its velocity: feasible."""
        s = p - rng.uniform(0.5, 0.9, N)
        th = uang + rng.uniform(-50, 50, N) * math.pi / 180
        el = rng.uniform(-0.3, 0.3, N)
        c = a.copy()
        c[:N] += s * np.cos(el) * np.cos(th)
        c[N:2 * N] += s * np.cos(el) * np.sin(th)
        c[2 * N:] += s * np.sin(el)
        return c

    def put(c, t):
        c[N - 1], c[2 * N - 1], c[3 * N - 1] = t[0], t[1], t[2]   # (anchor 0: the move itself)
        return c

    thr = pkg._lib.motion_thresholds
    q_hi, q_lo = thr(P_LAST, A_MAX)
    T5 = math.nextafter(4.0, INF)                  # dlim_threshold(2): sqrt(q3) > 2  <=>  q3 > 4 + 2^-50
    rows = [base(), a.copy()]                      # a feasible candidate; the zero move
    for T in (T5, q_hi, q_lo):
        for q in (math.nextafter(T, 0.0), T, math.nextafter(T, INF)):
            rows.append(put(base(), move_with_q3(q)))
    for tx, ty in cone_ladder(pkg):
        rows.append(put(base(), (tx, ty, 0.0)))
    for pos, v in ((N - 1, NAN), (N, INF), (2 * N, INF), (3 * N - 1, NAN), (0, -INF)):
        c = base()
        c[pos] = v
        rows.append(c)
    special = len(rows)                            # (19 rows so far; row k >= 19 is of kind k % 4)
    while len(rows) < K:                           # one planted violation in one UAV, by kind
        k = len(rows)
        c = base()
        i = (k * 37) % N
        kind = k % 4
        un = math.hypot(ux[i], uy[i])
        d = (ux[i] / un, uy[i] / un) if un > 0 else (1.0, 0.0)
        if kind == 1:      # speed (and acceleration): 2.5 along the velocity
            c[i], c[N + i], c[2 * N + i] = a[i] + 2.5 * d[0], a[N + i] + 2.5 * d[1], a[2 * N + i]
        elif kind == 2:    # acceleration alone: nearly no move (p > 1.05)
            c[i], c[N + i], c[2 * N + i] = a[i] + 0.01 * d[0], a[N + i] + 0.01 * d[1], a[2 * N + i]
        elif kind == 3:    # the cone alone: p straight back
            c[i], c[N + i], c[2 * N + i] = a[i] - p[i] * d[0], a[N + i] - p[i] * d[1], a[2 * N + i]
        rows.append(c)
    assert special == 19
    C = np.array(rows)
    _DATA[(N, K)] = (C, mo)
    return C, mo


def build_small(pkg, N):
    """K = 5: a feasible row, the zero move, and a planted row of each kind (rows 21, 22, 23)."""
    C, mo = build(pkg, N)
    return C[[0, 1, 21, 22, 23]], mo


def subset(mo, *names):
    keys = {"cons4": ("vel", "cone_cos"), "cons5": ("v_max",), "cons6": ("speed_prev", "a_max")}
    out = {"anchor": mo["anchor"]}
    for n in names:
        out.update({k: mo[k] for k in keys[n]})
    return out


def expected(pkg, C, mo, sample=None):
    """The yardstick's per-constraint masks, checked against the host callables (every candidate, or
    the rows `sample`), each with both classes."""
    y = yard(C, mo)
    fns = callables(pkg, mo)
    rows = range(C.shape[0]) if sample is None else sample
    for name, ok in y.items():
        assert ok.any() and not ok.all(), (name, "needs a rejected and a passing candidate")
        for k in rows:
            assert bool(fns[name](C[k])) == bool(ok[k]), (name, k)
    return y


SIZES = [1, 2, 8, 257, 513, 2048]


def _sample(N):
    return None if N <= 8 else [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 20, 21, 22, 23]


# ---------------------------------------------------------------- the ladders, on the host

def test_ladders_straddle_on_the_host(pkg):
    """The rows the device is probed with decide as intended on the host: at each threshold the
    pattern (below, at, above) is (pass, pass, reject) for cons5 and cons6's upper side,
    (reject, reject, pass) for cons6's lower side, and (reject, pass, pass) for the cone."""
    C, mo = build(pkg, 8)
    f = callables(pkg, mo)
    got5 = [bool(f["cons5"](C[k])) for k in (2, 3, 4)]
    hi6 = [bool(f["cons6"](C[k])) for k in (5, 6, 7)]
    lo6 = [bool(f["cons6"](C[k])) for k in (8, 9, 10)]
    cone = [bool(f["cons4"](C[k])) for k in (11, 12, 13)]
    assert got5 == [True, True, False] and hi6 == [True, True, False]
    assert lo6 == [False, False, True] and cone == [False, True, True]
    assert not f["cons6"](C[1]) and f["cons5"](C[1]) and f["cons4"](C[1])   # the zero move: |0 - p| > 1
    # a NaN x or r of the ladder UAV is feasible for it (rows 14, 17: the other UAVs make base moves)
    assert all(f[n](C[k]) for n in f for k in (14, 17))


# ---------------------------------------------------------------- the mask

@pytest.mark.parametrize("N", SIZES)
def test_mask_each_constraint_alone_and_together(ctx, pkg, N):
    C, mo = build(pkg, N)
    y = expected(pkg, C, mo, _sample(N))
    for name in ("cons4", "cons5", "cons6"):
        got = ctx.cons_mask(C, None, motion=subset(mo, name))
        assert np.array_equal(got, y[name]), (name, np.flatnonzero(got != y[name])[:8])
    allm = y["cons4"] & y["cons5"] & y["cons6"]
    assert allm.any() and not allm.all()
    got = ctx.cons_mask(C, None, motion=mo)
    assert np.array_equal(got, allm), np.flatnonzero(got != allm)[:8]
    # ... with cons8 (and cons7 off): the sorting kernel with the motion tests in its loader
    y8 = yard_cons8(C, mo["anchor"], 10.0)
    if N >= 2:
        assert not y8.all() and (allm & ~y8).any() and (allm & y8).any()
    got = ctx.cons_mask(C, {"d_sep": 10.0}, motion=mo)
    assert np.array_equal(got, allm & y8), np.flatnonzero(got != (allm & y8))[:8]
    assert np.array_equal(ctx.cons_mask(C, {"d_sep": 10.0}), y8)


def test_mask_k5_below_the_poll_chain(ctx, pkg):
    C, mo = build_small(pkg, 8)
    y = expected(pkg, C, mo)
    allm = y["cons4"] & y["cons5"] & y["cons6"]
    assert np.array_equal(ctx.cons_mask(C, None, motion=mo), allm)
    for name in y:
        assert np.array_equal(ctx.cons_mask(C, None, motion=subset(mo, name)), y[name])


# ---------------------------------------------------------------- the masked matrix poll

def _points(ctx, pkg):
    x, y, w = pkg.workloads.grid_points(64)
    ctx.set_points(x - 320.0, y - 320.0, w)


def _poll_case(ctx, pkg, C, mo, N):
    r_max = np.full(N, 6.0)
    c3 = dict(prev=mo["anchor"], d_lim=np.full(N, 2.2), tan_half_fov=TAN50)
    y = yard(C, mo)
    y8 = yard_cons8(C, mo["anchor"], 10.0)
    for motion, cons, kw, ok in (
            (subset(mo, "cons5"), None, {}, y["cons5"]),
            (mo, None, {}, y["cons4"] & y["cons5"] & y["cons6"]),
            (mo, {"d_sep": 10.0}, c3, y["cons4"] & y["cons5"] & y["cons6"] & y8)):
        bo0, bi0, obj0 = ctx.poll_best(C, r_max, 1e5, want_all=True, **kw)
        want = np.where(ok, obj0, INF)
        bo, bi, obj = ctx.poll_best(C, r_max, 1e5, want_all=True, cons=cons, motion=motion, **kw)
        # (the row with a NaN radius has a NaN objective in both polls)
        assert np.array_equal(obj, want, equal_nan=True), np.flatnonzero(obj != want)[:8]
        fin = np.flatnonzero(want < INF)
        if fin.size:
            k = int(fin[np.argmin(want[fin])])     # (np.argmin: the lowest index among equals)
            assert (bo, bi) == (want[k], k)
        else:
            assert (bo, bi) == (INF, -1)
        assert np.isfinite(want).any() and (~ok & np.isfinite(obj0)).any()   # the mask changes the poll


@pytest.mark.parametrize("N", SIZES)
def test_poll_best_under_motion(ctx, pkg, N):
    C, mo = build(pkg, N)
    _points(ctx, pkg)
    _poll_case(ctx, pkg, C, mo, N)


def test_poll_best_k5(ctx, pkg):
    C, mo = build_small(pkg, 8)
    _points(ctx, pkg)
    _poll_case(ctx, pkg, C, mo, 8)


# ---------------------------------------------------------------- off is off; the size limit

def test_off_is_off(ctx, pkg):
    C, mo = build(pkg, 8)
    _points(ctx, pkg)
    r_max = np.full(8, 6.0)
    off = [pkg._lib.Motion(), {"anchor": mo["anchor"]},
           dict(mo, cone_cos=NAN, v_max=NAN, a_max=NAN),
           {"anchor": mo["anchor"], "cone_cos": CONE, "a_max": A_MAX}]   # (no vel, no speed_prev: off)
    for cons in (None, {"d_sep": 10.0}):
        m0 = ctx.cons_mask(C, cons)
        p0 = ctx.poll_best(C, r_max, 1e5, want_all=True, cons=cons)
        for m in off:
            assert np.array_equal(ctx.cons_mask(C, cons, motion=m), m0)
            p = ctx.poll_best(C, r_max, 1e5, want_all=True, cons=cons, motion=m)
            assert p[:2] == p0[:2] and p[2].tobytes() == p0[2].tobytes()


def test_size_limit(ctx, pkg):
    N = 2049
    _points(ctx, pkg)
    a = np.zeros(3 * N)
    C = np.zeros((2, 3 * N))
    mo = {"anchor": a, "v_max": V_MAX}
    for call in (lambda: ctx.cons_mask(C, None, motion=mo),
                 lambda: ctx.poll_best(C, np.ones(N), 1e5, motion=mo)):
        with pytest.raises(pkg._lib.MaxCoverError) as e:
            call()
        assert e.value.code == pkg._lib.MAC_E_INVAL and "2048" in str(e.value)
