"""The cases of tests/test_gpu_verdicts.py, built and checked on the CPU: candidates, descriptors and
the expected records from the host mirror TDM_Constraints.explain (pinned by tests/test_verdict_host.py
against a brute force and the host callables). Every builder caches what it computes, so each
reference is computed once and shared."""
import math

import numpy as np

NAN, INF = float("nan"), float("inf")
FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)
KINDS = ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")
PITCH, D_SEP = 6.0, 5.0
ZONE_Y, ZONE_R = 103.0, 12.0
CONE, V_MAX, A_MAX, D_LIM = -0.5, 4.0, 3.0, 6.0

_CACHE = {}


def mirror(pkg, C, desc, prev=None, d_lim=None, tan=TAN50):
    """explain() of every row of C as one structured array."""
    ex = pkg.TDM_Constraints.explain
    out = np.zeros(len(C), dtype=pkg._lib.VERDICT_DTYPE)
    for k, c in enumerate(C):
        out[k] = ex(c, desc, prev=prev, d_lim=d_lim, tan_half_fov=tan)
    return out


def same(got, want):
    """Record-for-record equality, with the first difference in the message."""
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in range(len(want)):
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


# ---------------------------------------------------------------- case 1: all six kinds on

# which r move and which y moves candidate k plants (k = 0: the anchor itself, which passes everything)
#   r: +1 inside the zone -> cons7;  -4 -> cons6;  -5 -> cons5, cons6;  -8 -> cons3, cons5, cons6
#   y: +2 towards the next UAV of the row (4 < 5 apart) -> cons8;  -1 against the velocity (0, 1) ->
#      cons4 (and exactly 5 from the previous UAV: the strict boundary, no pair)
PLAN = {1: (-4.0, ("cons8",)), 2: (1.0, ()), 3: (-8.0, ("cons8",)), 4: (1.0, ("cons4",)),
        5: (-5.0, ("cons4", "cons8")), 6: (-8.0, ("cons4",))}


def matrix_case(pkg, N):
    """K = 7 seeded integer candidates over N UAVs on a lattice of pitch 6 with every kind on, the
    descriptors, and the mirror's records. Asserted here: every kind that can reject at this N
    rejects some candidates and not all."""
    key = ("matrix", N)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(7000 + N)
    side = max(1, math.ceil(math.sqrt(N)))
    ix, iy = np.divmod(np.arange(N), side)
    a = np.concatenate([100.0 + PITCH * ix, 100.0 + PITCH * iy, np.full(N, 12.0)])
    vel = np.concatenate([np.zeros(N), np.ones(N)])
    desc = dict(cons=dict(d_sep=D_SEP, zone_y=ZONE_Y, zone_r=ZONE_R),
                motion=dict(anchor=a, vel=vel, speed_prev=np.zeros(N), cone_cos=CONE, v_max=V_MAX, a_max=A_MAX))
    d_lim = np.full(N, D_LIM)
    in_zone = np.flatnonzero(iy == 0)
    has_next = np.flatnonzero((iy < side - 1) & (np.arange(N) + 1 < N))   # UAV i + 1 is PITCH above in y
    no_next = np.setdiff1d(np.arange(N), has_next)

    def pick(pool, used):
        pool = np.setdiff1d(pool, used) if N > 2 else pool
        m = min(len(pool), 1 + int(rng.integers(0, 3)))
        return rng.choice(pool, size=m, replace=False) if m else np.zeros(0, dtype=int)

    rows = [a.copy()]
    for k in range(1, 7):
        dr, ys = PLAN[k]
        c = a.copy()
        used = np.zeros(0, dtype=int)
        who = pick(in_zone if dr > 0 else np.arange(N), used)
        c[2 * N + who] += dr
        if N > 2:
            used = who
        for kind in ys:
            if kind == "cons8":
                who = pick(has_next, used)
                c[N + who] += 2.0
            else:
                who = pick(no_next if N > 1 else np.arange(N), used)
                c[N + who] -= 1.0
            used = np.concatenate([used, who, who + 1])
        rows.append(c)
    C = np.array(rows)
    assert np.array_equal(C, np.round(C))
    want = mirror(pkg, C, desc, prev=a, d_lim=d_lim)
    for q, kind in enumerate(KINDS):
        n = int(np.count_nonzero(want["reasons"] >> q & 1))
        if kind == "cons8" and N == 1:
            assert n == 0
        else:
            assert 0 < n < len(C), (N, kind, n)
    assert int(want["reasons"][0]) == 0
    _CACHE[key] = dict(C=C, desc=desc, prev=a, d_lim=d_lim, tan=TAN50, want=want)
    return _CACHE[key]


def only(desc, kind):
    """(cons, motion) with the one kind on (kinds 1-5), for Context.cons_mask."""
    c, m = desc["cons"], desc["motion"]
    if kind == "cons8":
        return {"d_sep": c["d_sep"]}, None
    if kind == "cons7":
        return {"zone_y": c["zone_y"], "zone_r": c["zone_r"]}, None
    keys = {"cons4": ("vel", "cone_cos"), "cons5": ("v_max",), "cons6": ("speed_prev", "a_max")}[kind]
    return None, {"anchor": m["anchor"], **{k: m[k] for k in keys}}


# ---------------------------------------------------------------- case 3: the sweep's edges

def line_case(pkg, N=600, d=15.0, shrink=False):
    """N UAVs on a line exactly d apart (no pair: the test is a strict <), spanning more than 256 d, so
    the cells are wider than the cut. shrink: UAV i = 1, 4, 7, ... moved one ulp towards UAV i - 1, so
    exactly the pairs (i - 1, i) violate."""
    x = d * np.arange(N)
    if shrink:
        x[1::3] = np.nextafter(x[1::3], -INF)
    C = np.concatenate([x, np.full(N, 50.0), np.full(N, 3.0)])[None, :]
    return C, {"d_sep": d}


def move_with_q3(q):
    """(tx, ty, tz), all > 0, with fl(fl(fl(tx*tx) + fl(ty*ty)) + fl(tz*tz)) == q exactly (tx, ty fp32
    values: their squares and the sum of the squares are exact doubles; tz the root of the rest)."""
    tx = float(np.float32(0.9 * math.sqrt(q)))
    ty = float(np.float32(math.sqrt(0.9 * (q - tx * tx))))
    tz = math.sqrt(q - (tx * tx + ty * ty))
    assert (tx * tx + ty * ty) + tz * tz == q, q
    return tx, ty, tz


U_LAD, P_LAD = (1.0, 0.25), 1.25   # the ladder UAV's velocity and speed_prev


def cone_ladder(pkg):
    """Moves (tx, ty) of the ladder UAV whose cosine is the double below -0.5, -0.5 and the double
    above: a host search over the ulps of ty around the 120-degree direction."""
    cc = pkg.TDM_Constraints.cone_cosine
    want = {CONE: None, math.nextafter(CONE, -INF): None, math.nextafter(CONE, INF): None}
    th = math.atan2(U_LAD[1], U_LAD[0]) + 2.0 * math.pi / 3.0
    rng = np.random.default_rng(4)
    for _ in range(400):
        r = float(rng.uniform(0.4, 1.2))
        tx, ty = r * math.cos(th), r * math.sin(th)
        for _ in range(48):
            ty = math.nextafter(ty, -INF)
        for _ in range(96):
            ty = math.nextafter(ty, INF)
            c = cc(U_LAD[0], U_LAD[1], tx, ty)
            if c in want and want[c] is None:
                want[c] = (tx, ty)
        if all(v is not None for v in want.values()):
            break
    assert all(v is not None for v in want.values()), want
    return [want[k] for k in sorted(want)]


def ladder_case(pkg):
    """N = 3: UAVs 0 and 1 carry the spacing ladder (d_sep = 15: one ulp inside, exactly at, one ulp
    outside), UAV 2 (anchor 0: its move is its coordinate) the ladders of v_max = 2 (q3 around
    dlim_threshold), a_max = 1 (both sides of cons6) and the cone's cosine around -0.5. Each row's
    expected reasons are stated here beside the mirror's records."""
    if "ladder" in _CACHE:
        return _CACHE["ladder"]
    a = np.array([100.0, 115.0, 0.0, 50.0, 50.0, 0.0, 6.0, 6.0, 0.0])
    vel = np.array([0.0, 0.0, U_LAD[0], 0.0, 0.0, U_LAD[1]])
    sp = np.array([0.0, 0.0, P_LAD])
    rows, reasons = [], []

    def row(x1=115.0, t=(0.0, 0.0, 0.0)):
        c = a.copy()
        c[1] = x1
        c[2], c[5], c[8] = t
        return c

    for x1, bit in ((math.nextafter(115.0, 0.0), 2), (115.0, 0), (math.nextafter(115.0, INF), 0)):
        rows.append(row(x1))
        reasons.append(bit | 0x20)   # (the ladder UAV stays: |0 - 1.25| > 1, cons6)
    q_hi, q_lo = pkg._lib.motion_thresholds(P_LAD, 1.0)
    T5 = math.nextafter(4.0, INF)    # sqrt(q3) > 2  <=>  q3 > 4 + 2^-50
    for T, below, at, above in ((T5, 0, 0, 0x10 | 0x20), (q_hi, 0, 0, 0x20), (q_lo, 0x20, 0x20, 0)):
        for q, bit in ((math.nextafter(T, 0.0), below), (T, at), (math.nextafter(T, INF), above)):
            rows.append(row(t=move_with_q3(q)))
            reasons.append(bit)
    for (tx, ty), bit in zip(cone_ladder(pkg), (0x08, 0, 0)):
        rows.append(row(t=(tx, ty, 0.0)))
        reasons.append(bit)
    C = np.array(rows)
    desc = dict(cons=dict(d_sep=15.0), motion=dict(anchor=a, vel=vel, speed_prev=sp, cone_cos=CONE, v_max=2.0, a_max=1.0))
    want = mirror(pkg, C, desc)
    # the speed and cone rows: whatever else the move does to the other motion kinds is the mirror's
    # word; the ladder's own bit is stated
    own = [0x02] * 3 + [0x10] * 3 + [0x20] * 6 + [0x08] * 3
    for k, (r, o) in enumerate(zip(reasons, own)):
        assert int(want["reasons"][k]) & o == r & o, (k, hex(int(want["reasons"][k])), hex(r))
    _CACHE["ladder"] = dict(C=C, desc=desc, want=want)
    return _CACHE["ladder"]


# ---------------------------------------------------------------- case 4: the driver's tallies

def _recipe(pkg, N, seed, lo, span, G=160):
    """tests/test_gpu_mads_cons.py's recipe."""
    wl = pkg.workloads
    x, y, w = wl.grid_points(G)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    rng = wl.SplitMix64(seed)
    x0 = np.concatenate([np.round(lo + rng.uniform(N) * span), np.round(lo + rng.uniform(N) * span),
                         np.full(N, 36.0)])
    return rec, x0, np.full(N, 30.0 * TAN50)


MADS = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
NATIVE = dict(n_iter=30, ell0=2, ell_max=5, seed=99)


def driver_case(pkg, orc, poll_vars="xyr", d_lim=10.0):
    """N = 12 under cons8(5.0), cons7, cons3 and a motion descriptor. Reference: TDM_STATIC_opt.mads over
    the oracle's objective with ONE host callable that evaluates every constraint for every trial point
    (explain: no short-circuit) and counts. The tally to compare is over the candidates of the polls
    the native driver launches: the start point is left out, and so is every poll that cons3 rejects
    whole by the driver's rule (include/maxcover.h rejected_polls: every polled variable's diagonal
    step +-2^ell alone exceeds its UAV's d_lim), restated here from the poll's own candidates; the native
    rejected_polls must equal `whole` (asserted by the test). d_lim = 3: the polls at steps 4 and
    above are rejected whole (asserted: some are, some are not)."""
    key = ("driver", poll_vars, d_lim)
    if key in _CACHE:
        return _CACHE[key]
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    N = 12
    rng = np.random.default_rng(12)
    c3 = TC.create_cons3(x0, FOV, np.full(N, d_lim))
    vel = np.concatenate([rng.integers(-2, 3, N), rng.integers(-2, 3, N)]).astype(np.float64)
    cons = [TC.create_cons8(5.0), TC.create_cons7(FOV, y_below=float(np.min(x0[N:2 * N])), h_above=30.0),
            c3, TC.create_cons4(vel, x0, CONE), TC.create_cons5(x0, 9.0), TC.create_cons6(x0, np.full(N, 2.0), 6.0)]
    recs, pts = [], []

    def every(v):
        r = TC.explain(v, cons)
        recs.append(int(r["reasons"]))
        pts.append(np.array(v, dtype=np.float64))
        return int(r["reasons"]) == 0

    def rejected_whole(X):
        """The candidates are x + B[:, k] and x - B[:, k] (integers: exact), |B| <= 2^ell on the diagonal."""
        n_p = len(X) // 2
        x = (X[0] + X[n_p]) / 2.0
        b = float(np.max(np.abs(X[:n_p] - x)))
        for v in range(n_p):
            q, i = divmod(v, N)
            for c in (x[v] + b, x[v] - b):
                d = c3.prev[v] - c if q < 2 else c3.prev[v] / c3.tan_half_fov - c / c3.tan_half_fov
                if not math.sqrt(d * d) > c3.d_lim[i]:
                    return False
        return True

    def objective(v):
        return orc.ref_objective(v, rec, r_max, 1e5)

    res = TS.mads(x0, objective, [every], poll_vars=poll_vars, **MADS)
    K = 2 * TS.polled_count(x0.size, poll_vars)
    it = res.status.iteration
    assert len(recs) == 1 + it * K
    polls = np.array(recs[1:], dtype=np.int64).reshape(it, K)
    X = np.array(pts[1:]).reshape(it, K, x0.size)
    whole = np.array([rejected_whole(X[t]) for t in range(it)])
    assert np.all(polls[whole] & 1 != 0)   # (such a poll's candidates all fail cons3)
    live = polls[~whole]
    tally = dict(candidates=int(live.size), rejected_any=int(np.count_nonzero(live)),
                 rejected_by={k: int(np.count_nonzero(live >> q & 1)) for q, k in enumerate(KINDS)},
                 polls=int(live.shape[0]))
    # the case is worth its time: every kind rejects some of the launched candidates and not all
    for k in KINDS if d_lim == 10.0 else ("cons3",):
        assert 0 < tally["rejected_by"][k] < tally["candidates"], (k, tally)
    if d_lim != 10.0:
        assert 0 < np.count_nonzero(whole) < it
    assert 0 < tally["rejected_any"] < tally["candidates"]
    cm, _ = TC.merge_mac_cons(cons)
    mm, _ = TC.merge_mac_motion(cons)
    out = dict(rec=rec, x0=x0, r_max=r_max, tally=tally, whole=int(np.count_nonzero(whole)), it=it,
               x=res.x if res.x is not None else res.i, f=res.x_cost if res.x is not None else math.inf,
               evals=res.status.function_evaluations, polls=polls, K=K,
               kw=dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, cons=cm, motion=mm,
                       poll_vars=poll_vars, **NATIVE))
    _CACHE[key] = out
    return out
