"""Mirror of the extreme constraints the driver passes to MADS (src/TDM_Constraints.jl):
``cons1`` (:9-19, always true) and ``create_cons3`` (:54-75, per-UAV 3-D displacement limit).
The returned ``cons3`` evaluates on the host with the reference's arithmetic and also carries
its data (``prev``, ``d_lim``, ``tan_half_fov``) so the batched GPU poll can apply the same
test inside libmaxcover (finalize kernel, exact threshold form).

``create_cons8`` (:157-172, minimum spacing) and ``create_cons7`` (:142-154, altitude zone) are the
swarm constraints written for the reference's ``cons_ext`` slot; they carry ``mac_cons`` fields, which
``TDM_STATIC_opt.mads`` merges into one descriptor for the device (include/maxcover.h mac_cons).

``create_cons4`` (:78-103, velocity cone), ``create_cons5`` (:106-119, target speed) and
``create_cons6`` (:122-138, target acceleration) limit the move away from the previous target; they
carry ``mac_motion`` fields, merged the same way (include/maxcover.h mac_motion).

``create_cons1_progressive`` (:182-195) and ``create_cons_progressive`` (:197-219) are the
progressive constraints of the reference's ``cons_prog`` slot: host callables returning the altitude
excess c(x) >= 0, carrying ``mac_prog`` fields that ``merge_mac_prog`` turns into one descriptor
(include/maxcover.h mac_prog) for the progressive barrier of ``TDM_STATIC_opt.mads(cons_prog=)`` and
``Context.mads_run(prog=)``."""
from __future__ import annotations

import math

import numpy as np


def cons1(x) -> bool:
    """src/TDM_Constraints.jl:9-19 — the body is commented out; always feasible."""
    return True


def _cons3_rejects(prev, t: float, dl, xx, N: int, i: int) -> bool:
    """UAV i's own cons3 test (:61-70): its 3-D move from ``prev`` is longer than ``dl[i]``."""
    x1, y1, z1 = float(prev[i]), float(prev[N + i]), float(prev[2 * N + i]) / t
    x2, y2, z2 = float(xx[i]), float(xx[N + i]), float(xx[2 * N + i]) / t
    return math.sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2)) > dl[i]


def create_cons3(pre_optimized_circles_MADS, FOV: float, d_lim):
    """src/TDM_Constraints.jl:54-75. ``pre_optimized_circles_MADS``: list of Circle or [x;y;R]."""
    from .AreaCoverageCalculation import make_MADS
    pre = pre_optimized_circles_MADS
    if len(pre) and not isinstance(pre[0], (float, int, np.floating, np.integer)):
        prev = make_MADS(pre)
    else:
        prev = np.asarray(pre, dtype=np.float64)
    prev = np.ascontiguousarray(prev, dtype=np.float64)
    dl = np.ascontiguousarray(np.asarray(d_lim, dtype=np.float64))
    t = math.tan(FOV / 2)

    def cons3(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            if _cons3_rejects(prev, t, dl, xx, N, i):
                return False
        return True

    cons3.prev = prev
    cons3.d_lim = dl
    cons3.tan_half_fov = t
    return cons3


def _cons7_rejects(y_lim: float, r_lim: float, xx, N: int, i: int) -> bool:
    """UAV i's own cons7 test (:146-150): inside the zone and above its cap."""
    return float(xx[i + N]) < y_lim and float(xx[i + 2 * N]) > r_lim


def create_cons7(FOV: float, y_below: float = 200.0, h_above: float = 19.0):
    """src/TDM_Constraints.jl:142-154 (altitude cap inside a zone): infeasible when a UAV with
    y < y_below has R > h_above * tan(FOV/2). The reference reads N, FOV and the two numbers from
    its globals; here they are arguments. Carries ``mac_cons`` (zone_y, zone_r) for the device."""
    y_lim = float(y_below)
    r_lim = float(h_above) * math.tan(FOV / 2)

    def cons7(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            if _cons7_rejects(y_lim, r_lim, xx, N, i):
                return False
        return True

    cons7.mac_cons = {"zone_y": y_lim, "zone_r": r_lim}
    return cons7


def _cons8_pair(d: float, xx, N: int, i: int, j: int) -> bool:
    """cons8's test of the pair (i, j) (:162-166): closer than ``d`` horizontally."""
    dx = float(xx[i]) - float(xx[j])
    dy = float(xx[i + N]) - float(xx[j + N])
    hor_separation = math.sqrt(dx * dx + dy * dy)
    return hor_separation < d


def create_cons8(d_sep: float = 15.0):
    """src/TDM_Constraints.jl:157-172 (minimum horizontal spacing between any two UAVs), 15.0 in
    the reference. Carries ``mac_cons`` (d_sep) for the device."""
    d = float(d_sep)

    def cons8(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            for j in range(N):
                if j != i and _cons8_pair(d, xx, N, i, j):
                    return False
        return True

    cons8.mac_cons = {"d_sep": d}
    return cons8


def _anchor(anchor) -> np.ndarray:
    """[x; y; R] (3N doubles) from a list of Circle or the vector itself."""
    from .AreaCoverageCalculation import make_MADS
    a = anchor
    if len(a) and not isinstance(a[0], (float, int, np.floating, np.integer)):
        a = make_MADS(a)
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())


def _move(xx, a, N: int, i: int):
    """UAV i's move t = x - a and q2 = fl(fl(tx*tx) + fl(ty*ty)) (Python floats: IEEE, no FMA)."""
    tx = float(xx[i]) - float(a[i])
    ty = float(xx[N + i]) - float(a[N + i])
    tz = float(xx[2 * N + i]) - float(a[2 * N + i])
    return tx, ty, tz, tx * tx + ty * ty


def _sqrt(q: float) -> float:
    return math.sqrt(q) if q >= 0.0 and q != math.inf else float(np.sqrt(np.float64(q)))


def cone_cosine(ux: float, uy: float, tx: float, ty: float) -> float:
    """cons4's c = dot(u, t) / (|u| |t|) in the device's plain form (include/maxcover.h mac_motion);
    0/0 (a zero velocity or a zero move) and inf/inf give NaN, as IEEE division does."""
    q2 = tx * tx + ty * ty
    with np.errstate(all="ignore"):
        den = np.float64(_sqrt(ux * ux + uy * uy)) * np.float64(_sqrt(q2))
        return float(np.float64(ux * tx + uy * ty) / den)


def _cons4_rejects(a, v, cc: float, xx, N: int, i: int) -> bool:
    """UAV i's own cons4 test: its move leaves the cone around its velocity (NaN: feasible)."""
    tx, ty, _, _ = _move(xx, a, N, i)
    return cone_cosine(float(v[i]), float(v[N + i]), tx, ty) < cc


def _cons5_rejects(a, vm: float, xx, N: int, i: int) -> bool:
    """UAV i's own cons5 test: its 3-D move from the anchor is longer than v_max."""
    _, _, tz, q2 = _move(xx, a, N, i)
    return _sqrt(q2 + tz * tz) > vm


def _cons6_rejects(a, sp, am: float, xx, N: int, i: int) -> bool:
    """UAV i's own cons6 test: its speed differs from speed_prev[i] by more than a_max."""
    _, _, tz, q2 = _move(xx, a, N, i)
    return abs(_sqrt(q2 + tz * tz) - float(sp[i])) > am


def create_cons4(velocities, anchor, cone_cos: float = -0.5):
    """src/TDM_Constraints.jl:78-103 (the target stays inside a cone around the UAV's xy velocity,
    "to reduce oscillatory target setting"). ``velocities``: [vx; vy] (2N values);
    ``anchor``: the previous MADS target, [x; y; R] or Circles. The reference's
    ``abs(acosd(round(c))) > 90`` is ``c < -0.5`` (round is ties-to-even), hence the default.
    Carries ``mac_motion`` (anchor, vel, cone_cos) for the device."""
    a = _anchor(anchor)
    N = a.size // 3
    v = np.ascontiguousarray(np.asarray(velocities, dtype=np.float64).ravel())
    if v.size != 2 * N:
        raise ValueError("velocities: 2N values [vx; vy]")
    cc = float(cone_cos)

    def cons4(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        for i in range(N):
            if _cons4_rejects(a, v, cc, xx, N, i):
                return False
        return True

    cons4.mac_motion = {"anchor": a, "vel": v, "cone_cos": cc}
    return cons4


def create_cons5(anchor, v_max: float = 2.0):
    """src/TDM_Constraints.jl:106-119 (target speed): infeasible when some UAV's 3-D move from
    ``anchor`` is longer than ``v_max`` (2 in the reference). Carries ``mac_motion``."""
    a = _anchor(anchor)
    N = a.size // 3
    vm = float(v_max)

    def cons5(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        for i in range(N):
            if _cons5_rejects(a, vm, xx, N, i):
                return False
        return True

    cons5.mac_motion = {"anchor": a, "v_max": vm}
    return cons5


def create_cons6(anchor, speed_prev, a_max: float = 1.0):
    """src/TDM_Constraints.jl:122-138 (target acceleration): infeasible when some UAV's speed
    |x - anchor| differs from ``speed_prev[i]`` (the norm of its previous target velocity) by more
    than ``a_max`` (1 in the reference). Carries ``mac_motion``."""
    a = _anchor(anchor)
    N = a.size // 3
    sp = np.ascontiguousarray(np.asarray(speed_prev, dtype=np.float64).ravel())
    if sp.size != N:
        raise ValueError("speed_prev: N values")
    am = float(a_max)

    def cons6(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        for i in range(N):
            if _cons6_rejects(a, sp, am, xx, N, i):
                return False
        return True

    cons6.mac_motion = {"anchor": a, "speed_prev": sp, "a_max": am}
    return cons6


def merge_mac_motion(constraints):
    """One mac_motion dict {anchor, vel, speed_prev, cone_cos, v_max, a_max} out of the callables
    that carry ``mac_motion`` data (None when there is none), and the list of the callables that do
    not. The descriptor has one anchor and one slot per kind: a constraint of a kind already taken,
    or around another anchor, stays a host callable."""
    merged, plain = {}, []
    for c in constraints:
        data = getattr(c, "mac_motion", None)
        if data and not ((set(data) - {"anchor"}) & set(merged)) and \
                ("anchor" not in merged or np.array_equal(merged["anchor"], data["anchor"],
                                                          equal_nan=True)):
            merged.update(data)
        else:
            plain.append(c)
    return (merged or None), plain


def merge_mac_cons(constraints):
    """One mac_cons dict {d_sep, zone_y, zone_r} out of the callables that carry ``mac_cons`` data
    (None when there is none), and the list of the callables that do not. Two constraints of one
    kind cannot share the descriptor's single slot: the later one stays a host callable."""
    merged, plain = {}, []
    for c in constraints:
        data = getattr(c, "mac_cons", None)
        if data and not (set(data) & set(merged)):
            merged.update(data)
        else:
            plain.append(c)
    return (merged or None), plain


# ---- verdicts: what rejects a trial point (include/maxcover.h mac_verdict)

VERDICT_KINDS = ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")   # kind q = bit q of reasons


def _descriptors(given):
    """(mac_cons dict or None, mac_motion dict or None, cons3 data or None) from None, a mapping
    (the mac_cons / mac_motion fields themselves, or under "cons" / "motion"), or callables that carry
    ``mac_cons`` / ``mac_motion`` data or create_cons3's ``prev`` / ``d_lim`` / ``tan_half_fov``."""
    if given is None:
        return None, None, None
    if hasattr(given, "get"):
        cons, motion = given.get("cons"), given.get("motion")
        if cons is None and motion is None:
            cons = {k: given[k] for k in ("d_sep", "zone_y", "zone_r") if given.get(k) is not None}
            motion = {k: given[k] for k in ("anchor", "vel", "speed_prev", "cone_cos", "v_max", "a_max")
                      if given.get(k) is not None}
        return (cons or None), (motion or None), None
    cs = list(given)
    cons, rest = merge_mac_cons(cs)
    motion, rest = merge_mac_motion(rest)
    c3 = next((c for c in rest if hasattr(c, "prev") and hasattr(c, "d_lim")), None)
    return cons, motion, c3


def explain(x, constraints=None, prev=None, d_lim=None, FOV: float = math.pi / 2, tan_half_fov=None):
    """What rejects the trial point ``x`` = [x; y; R]: one record of ``_lib.VERDICT_DTYPE``, the
    documented meaning of the device's mac_verdict (Context.cons_explain gives the same record).

    ``constraints``: the callables of this module (create_cons3 / 4 / 5 / 6 / 7 / 8; one of each
    kind), or a mapping of mac_cons / mac_motion fields. cons3 may also be given as ``prev``, ``d_lim``
    and ``FOV`` (or ``tan_half_fov`` itself). Every constraint that is on is evaluated in full, with
    the per-UAV and per-pair tests the callables themselves apply; none short-circuits another:
      reasons       bit q set iff kind q (VERDICT_KINDS) is on and rejects x, i.e. iff
                    ``not create_consq(...)(x)``
      n_uav[q]      the UAVs whose own test fails (cons8: the UAVs in at least one violating pair)
      first_uav[q]  the lowest of them, -1 when none
      pairs         cons8's unordered pairs i < j closer than d_sep
    A kind that is off (no data; d_sep <= 0 or NaN; a NaN bound; a missing array) has its bit clear,
    its counts 0 and first_uav -1. A UAV with a non-finite x or y is in no pair; a NaN operand
    rejects nothing."""
    from ._lib import VERDICT_DTYPE
    xx = np.asarray(x, dtype=np.float64).ravel()
    N = xx.size // 3
    cons, motion, c3 = _descriptors(constraints)
    bad = [[] for _ in VERDICT_KINDS]   # per kind: the UAVs whose own test fails, ascending
    pairs = 0
    nan = float("nan")
    if c3 is not None and prev is None:
        prev, d_lim, tan_half_fov = c3.prev, c3.d_lim, c3.tan_half_fov
    if prev is not None:
        if d_lim is None:
            raise ValueError("prev given without d_lim")
        pv = np.asarray(prev, dtype=np.float64).ravel()
        dl = np.asarray(d_lim, dtype=np.float64).ravel()
        t = math.tan(FOV / 2) if tan_half_fov is None else float(tan_half_fov)
        bad[0] = [i for i in range(N) if _cons3_rejects(pv, t, dl, xx, N, i)]
    if cons:
        d = float(cons.get("d_sep", nan) if cons.get("d_sep") is not None else nan)
        zy = float(cons.get("zone_y", nan) if cons.get("zone_y") is not None else nan)
        zr = float(cons.get("zone_r", nan) if cons.get("zone_r") is not None else nan)
        if d > 0.0 and N > 1:
            # _cons8_pair's test, restated on purpose: a Python call per pair is 2 million calls at
            # N = 2048. numpy's subtract, multiply, add and sqrt round each result as the float
            # operations do (no FMA), so UAV i against every j is the same test (pinned against
            # create_cons8 and a per-pair loop in tests/test_verdict_host.py). 256 rows at a time.
            px, py = xx[:N], xx[N:2 * N]
            for i0 in range(0, N, 256):
                i1 = min(i0 + 256, N)
                with np.errstate(all="ignore"):
                    dx = px[i0:i1, None] - px[None, :]
                    dy = py[i0:i1, None] - py[None, :]
                    close = np.sqrt(dx * dx + dy * dy) < d
                rows = np.arange(i0, i1)
                close[rows - i0, rows] = False                      # j != i
                pairs += int(np.count_nonzero(close & (np.arange(N)[None, :] > rows[:, None])))
                bad[1] += [int(i) for i in i0 + np.flatnonzero(close.any(axis=1))]
        if zy == zy and zr == zr:
            bad[2] = [i for i in range(N) if _cons7_rejects(zy, zr, xx, N, i)]
    if motion and motion.get("anchor") is not None:
        a = _anchor(motion["anchor"])
        v, sp = motion.get("vel"), motion.get("speed_prev")
        cc, vm, am = (float(motion[k]) if motion.get(k) is not None else nan
                      for k in ("cone_cos", "v_max", "a_max"))
        if cc == cc and v is not None:
            v = np.asarray(v, dtype=np.float64).ravel()
            bad[3] = [i for i in range(N) if _cons4_rejects(a, v, cc, xx, N, i)]
        if vm == vm:
            bad[4] = [i for i in range(N) if _cons5_rejects(a, vm, xx, N, i)]
        if am == am and sp is not None:
            sp = np.asarray(sp, dtype=np.float64).ravel()
            bad[5] = [i for i in range(N) if _cons6_rejects(a, sp, am, xx, N, i)]
    rec = np.zeros((), dtype=VERDICT_DTYPE)
    rec["pairs"] = pairs
    for q, b in enumerate(bad):
        rec["n_uav"][q] = len(b)
        rec["first_uav"][q] = b[0] if b else -1
        if b:
            rec["reasons"] |= np.uint32(1 << q)
    return rec


# ---- progressive constraints (src/TDM_Constraints.jl:182-220): altitude excess, handed to MADS's
# progressive barrier (src/TDM_STATIC_opt.jl:142-159) instead of the extreme one

def prog_term(R, limit) -> float:
    """Julia's ``max(R - limit, 0.0)``: a NaN difference stays NaN (fmax and Python's max drop it)."""
    d = float(R) - float(limit)
    return d if (d > 0.0 or d != d) else 0.0


def prog_h(c_values) -> float:
    """h = sum_j c_j * c_j folded from 0.0 in the order j = 0, 1, ...; each product is rounded
    before its add (Python floats: no FMA)."""
    h = 0.0
    for c in c_values:
        c = float(c)
        h = h + c * c
    return h


def _progressive(uavs, r_max):
    def c(x) -> float:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        rm = np.asarray(r_max, dtype=np.float64)   # read at call time, as createObjective does
        s = 0.0
        for i in (range(N) if uavs is None else uavs):          # :186-190
            s = s + prog_term(xx[2 * N + i], rm[i])
        return s

    c.mac_prog = {"uavs": uavs, "limit": r_max}
    return c


def create_cons1_progressive(r_max):
    """src/TDM_Constraints.jl:182-195: c(x) = sum_i max(R_i - r_max_i, 0) over every UAV, folded in
    the order i = 0..N-1. ``r_max`` is read at call time. Carries ``mac_prog`` data (every UAV a
    member, limit = r_max) for the device (include/maxcover.h mac_prog)."""
    return _progressive(None, r_max)


def create_cons_progressive(i: int, r_max):
    """src/TDM_Constraints.jl:197-219 (cons2_progressive, cons3_progressive): the altitude excess
    max(R_i - r_max_i, 0) of the single UAV ``i`` (0-based). Carries ``mac_prog`` data."""
    i = int(i)
    if i < 0:
        raise ValueError("create_cons_progressive: i is a 0-based UAV index")
    return _progressive((i,), r_max)


MAC_PROG_MAX = 32   # constraints one mac_prog holds (a bit per constraint in member[i])


def merge_mac_prog(constraints, N: int | None = None):
    """One mac_prog mapping {member, limit, n_cons} out of the callables that carry ``mac_prog``
    data (None when there is none), and the list of the callables that do not. Constraint j is the
    j-th of ``constraints``: bit j of member[i] says UAV i belongs to it. The descriptor has one
    limit per UAV, read from the constraints' ``r_max`` now; a constraint whose limits differ from
    the first one's, or the 33rd, stays a host callable. ``N``: the UAV count (default: the limits'
    length)."""
    member = limit = None
    plain, j = [], 0
    for c in constraints:
        data = getattr(c, "mac_prog", None)
        lim = None if data is None else np.asarray(data["limit"], dtype=np.float64).ravel()
        if lim is not None and N is not None:
            lim = lim[:N] if lim.size >= N else None
        if lim is None or j >= MAC_PROG_MAX or \
                (limit is not None and not np.array_equal(limit, lim, equal_nan=True)) or \
                (data["uavs"] is not None and any(u >= lim.size for u in data["uavs"])):
            plain.append(c)
            continue
        if limit is None:
            limit = np.ascontiguousarray(lim.copy())
            member = np.zeros(limit.size, dtype=np.uint32)
        if data["uavs"] is None:
            member |= np.uint32(1 << j)
        else:
            for u in data["uavs"]:
                member[u] |= np.uint32(1 << j)
        j += 1
    if limit is None:
        return None, plain
    return {"member": member, "limit": limit, "n_cons": j}, plain
