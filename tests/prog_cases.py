"""Shared by tests/test_prog_host.py and tests/test_gpu_prog.py: the recipes of the progressive-
barrier tests and the rule (DESIGN.md section 4 "Progressive barrier") written out one trial point
at a time, independently of TDM_STATIC_opt.mads_prog: plain loops, Python floats (IEEE doubles,
no FMA)."""
import math

import numpy as np

FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)
KW = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
_cache = {}


def grid_rec(pkg, G=160):
    if ("rec", G) not in _cache:
        x, y, w = pkg.workloads.grid_points(G)
        _cache["rec", G] = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    return _cache["rec", G]


def recipe(pkg, N, seed, lo, span, radii):
    """(rec, x0, r_max): integer positions from SplitMix64(seed), equal radii, r_max = 30 tan 50 deg
    (tests/test_granularity_host.py's N = 3 recipe is recipe(pkg, 3, 7, 320, 40, 36.0))."""
    rng = pkg.workloads.SplitMix64(seed)
    x0 = np.concatenate([np.round(lo + rng.uniform(N) * span), np.round(lo + rng.uniform(N) * span),
                         np.full(N, float(radii))])
    return grid_rec(pkg), x0, np.full(N, 30.0 * TAN50)


def term(R, limit):
    d = float(R) - float(limit)
    if d != d:
        return d          # Julia's max keeps the NaN
    return d if d > 0.0 else 0.0


def h_written_out(v, member, limit, J):
    """h of one point: c_j folded over i = 0..N-1 from 0.0, h folded over j = 0..J-1 from 0.0."""
    N = len(limit)
    h = 0.0
    for j in range(J):
        c = 0.0
        for i in range(N):
            if (int(member[i]) >> j) & 1:
                c = c + term(v[2 * N + i], limit[i])
        sq = c * c
        h = h + sq
    return h


def rule_written_out(pkg, obj, cons, member, limit, J, x0, g, n, N_iter, ell0, ell_max, seed, h_max0=None):
    """The rule, one trial point and one variable at a time. Returns a dict: per-iteration records
    (outcome, F.x, F.f, I.x, I.f, I.h, h_max, centres), the final F / I / h_max, the counts."""
    wl = pkg.workloads
    rng = wl.SplitMix64(seed)
    x0 = np.asarray(x0, dtype=np.float64)
    h0 = h_written_out(x0, member, limit, J)
    assert h0 == h0
    f0 = obj(x0) if all(c(x0) for c in cons) else math.inf
    F = (x0.copy(), f0) if h0 == 0.0 else None
    I = None if h0 == 0.0 else (x0.copy(), f0, h0)
    if h_max0 is not None and h_max0 >= 0.0:
        h_max = float(h_max0)
    else:
        h_max = h0 if h0 > 0.0 else math.inf
    assert not h0 > h_max
    ell, it = ell0, 0
    out = dict(iters=[], dominating=0, improving=0, unsuccessful=0, two=0, evaluated=0, evals=1)
    while it < N_iter and ell >= 0:
        it += 1
        B = wl.ltmads_basis(n, ell, rng)
        centres = [p[0] for p in (F, I) if p is not None]
        out["two"] += len(centres) == 2
        obj_c = [None, None]   # per centre: the objective of every trial point, +inf where it was dropped
        h_c = [None, None]
        points = {}
        for c, xc in enumerate(centres):
            obj_c[c], h_c[c] = [math.inf] * (2 * n), [math.nan] * (2 * n)
            for k in range(2 * n):
                out["evals"] += 1
                kk = k if k < n else k - n
                v = xc.copy()
                for q in range(n):
                    d = float(B[q, kk]) if g is None else float(g[q]) * float(B[q, kk])
                    v[q] = xc[q] + d if k < n else xc[q] - d
                if not all(cc(v) for cc in cons):
                    continue
                h = h_written_out(v, member, limit, J)
                if h != h or h > h_max:
                    continue
                out["evaluated"] += 1
                obj_c[c][k], h_c[c][k] = obj(v), h
                points[c * 2 * n + k] = v
        # 3-7
        code, _, bestF_g, newI_f, newI_h, newI_g, h_new, _ = select_written_out(
            None if F is None else F[1], None if I is None else I[1], None if I is None else I[2], h_max,
            obj_c, h_c, 2 * n)
        if code & 256:
            F = (points[bestF_g].copy(), obj_c[bestF_g // (2 * n)][bestF_g % (2 * n)])
        if newI_g >= 0:
            I = (points[newI_g].copy(), newI_f, newI_h)
        elif newI_g == NEW_I_NONE:
            I = None
        h_max = h_new
        dominating, improving = (code & 255) == 0, (code & 255) == 1
        if dominating:
            ell = min(ell + 1, ell_max)
            outcome = "dominating"
        elif improving:
            outcome = "improving"
        else:
            ell -= 1
            outcome = "unsuccessful"
        out[outcome] += 1
        out["iters"].append((outcome, None if F is None else F[0].copy(), None if F is None else F[1],
                             None if I is None else I[0].copy(), None if I is None else I[1],
                             None if I is None else I[2], h_max, len(centres)))
    out.update(F=F, I=I, h_max=h_max, it=it, status="MeshPrecisionLimit" if ell < 0 else "IterationLimit")
    return out


# ---------------------------------------------------------------- steps 3-7 alone: prog_select_kernel's record

NEW_I_NONE, NEW_I_OLD = -1, -2   # ProgRec.newI_g (k_prog.h kProgNone, kProgOld)
REPLACES_F = 256                 # ProgRec.outcome bit 8
INF = math.inf


def select_written_out(F_f, I_f, I_h, h_max, obj, h, K):
    """Steps 3-7 of DESIGN.md section 4 over the two per-centre arrays ``obj[c]`` / ``h[c]`` (K values
    each, or None: the centre was not polled), one candidate at a time; F_f None: no F, I_f / I_h None:
    no I. An objective of +inf means "not evaluated"; a NaN one is counted and selects nothing.
    Returns ProgRec's eight fields (k_prog.h): (outcome | 256 when bestF replaces F, bestF_f, bestF_g
    (-1: none; reported even when it does not improve), newI_f, newI_h, newI_g (-1: none, -2: the
    old one), h_new, evaluated)."""
    trial = []   # (f, h, g) in g = c K + k order: what was evaluated to a number
    evaluated = 0
    for c in (0, 1):
        if obj[c] is None:
            continue
        for k in range(K):
            f = float(obj[c][k])
            if f == math.inf:
                continue
            evaluated += 1
            if f != f:
                continue
            trial.append((f, float(h[c][k]), c * K + k))
    # 3: the best feasible trial point, the first in g order among equals
    bestF = None
    for t in trial:
        if t[1] == 0.0 and (bestF is None or t[0] < bestF[0]):
            bestF = t
    improves = bestF is not None and (F_f is None or bestF[0] < F_f)
    # 4, 5
    dominating = improves
    improving = False
    if I_h is not None:
        for f, hh, _ in trial:
            if hh > 0.0 and hh <= I_h and f <= I_f and (hh < I_h or f < I_f):
                dominating = True
        if not dominating:
            for f, hh, _ in trial:
                if hh > 0.0 and hh < I_h:
                    improving = True
    # 7
    if improving:
        h_new = max(hh for f, hh, _ in trial if hh > 0.0 and hh < I_h)
    else:
        h_new = I_h if I_h is not None else h_max
    newI = (I_f, I_h, NEW_I_OLD) if (I_h is not None and I_h <= h_new) else None
    for f, hh, g in trial:
        if hh > 0.0 and hh <= h_new:
            if newI is None or f < newI[0] or (f == newI[0] and hh < newI[1]):
                newI = (f, hh, g)
    code = (0 if dominating else 1 if improving else 2) | (REPLACES_F if improves else 0)
    bf = (math.inf, -1) if bestF is None else (bestF[0], bestF[2])
    ni = (math.inf, math.inf, NEW_I_NONE) if newI is None else newI
    return (code, bf[0], bf[1], ni[0], ni[1], ni[2], h_new, evaluated)


def record_bytes(rec):
    """A record as ProgRec's 64 bytes (NaN fields compare by their bits)."""
    import struct
    return struct.pack("<qdqddqdq", int(rec[0]), float(rec[1]), int(rec[2]), float(rec[3]), float(rec[4]),
                       int(rec[5]), float(rec[6]), int(rec[7]))


def rule_args(case):
    """(F_f, I_f, I_h, h_max) as the host rule takes them: None for an incumbent that does not exist."""
    return (case["F_f"] if case["has_F"] else None, case["I_f"] if case["has_I"] else None,
            case["I_h"] if case["has_I"] else None, case["h_max"])


SELECT_KS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 3072, 6600)
CENTRES = ("0", "1", "both")
F_LEVELS = (-60.0, -45.5, -45.0, -30.25, -10.0, 0.0)
H_LEVELS = (0.125, 0.5, 2.0, 9.0)


def _gen_case(rng, K, centres, has_F, has_I, share, bias):
    """One generated case. share: the part of the candidates left unevaluated (0, 0.5, "most": all
    but one or two, 1). bias: towards the improving outcome (an I, no candidate at or below I.f with
    h <= I.h, no feasible candidate below F.f)."""
    lv = np.array(F_LEVELS)
    I_h = float(rng.choice(H_LEVELS[1:]))
    if has_I:
        h_max = float(rng.choice([I_h, 16.0, INF]))
        I_f = float(rng.choice(list(lv[:-1] if bias else lv) + ([] if bias else [INF, math.nan])))
    else:
        h_max = float(rng.choice([2.0, 16.0, INF]))
        I_f = float(rng.choice(lv))   # (stale values: the kernel must not read them without has_I)
    F_f = float(lv[0]) if (bias and has_F) else float(rng.choice(list(lv) + [INF]))
    hs = np.array([0.0, 5e-324] + list(H_LEVELS) + [12.0, I_h, np.nextafter(I_h, -INF), np.nextafter(I_h, INF)])
    obj, h = [None, None], [None, None]
    for c in (0, 1):
        if centres != "both" and centres != str(c):
            continue
        hc = rng.choice(hs, K)
        fc = rng.choice(np.concatenate([lv, [math.nan]]), K, p=[0.16] * 6 + [0.04])
        if bias:
            if not has_F:
                hc = np.where(hc == 0.0, 5e-324, hc)
            low = (hc > 0.0) & (hc <= I_h) & ~(fc > I_f)   # (NaN included)
            fc = np.where(low, lv[-1], fc)
        if share == "most":
            keep = np.zeros(K, dtype=bool)
            keep[rng.integers(0, K, 2)] = True
        else:
            keep = rng.random(K) >= share
        # a candidate above the barrier is never evaluated; a fifth of those above h_max were cut by it
        above = rng.random(K) < 0.2
        hc = np.where(above & np.isfinite(h_max), 2.0 * h_max + 1.0, hc)
        fc = np.where(keep & ~(hc > h_max), fc, INF)
        obj[c], h[c] = np.ascontiguousarray(fc), np.ascontiguousarray(hc)
    return dict(K=K, obj=obj, h=h, has_F=int(has_F), has_I=int(has_I), F_f=F_f, I_f=I_f, I_h=I_h if has_I else 0.75,
                h_max=h_max, want=None)


def _blank(K, both=False):
    """Arrays of a hand-written case: nothing evaluated (objective +inf, h = 1.0)."""
    mk = lambda: (np.full(K, INF), np.full(K, 1.0))   # noqa: E731
    (o0, h0), (o1, h1) = mk(), mk()
    return [o0, o1 if both else None], [h0, h1 if both else None]


def _hand_cases():
    """Each with its answer in ``want`` (ProgRec's eight fields), worked out by hand from the rule."""
    out = []
    below3 = np.nextafter(-3.0, -INF)

    def add(name, K, obj, h, want, F=None, I=None, h_max=INF):
        out.append(dict(name=name, K=K, obj=obj, h=h, has_F=int(F is not None), has_I=int(I is not None),
                        F_f=-1e9 if F is None else F, I_f=-1e9 if I is None else I[0],
                        I_h=0.75 if I is None else I[1], h_max=h_max, want=want))

    # the minimal f twice among feasible candidates: the lowest g wins
    o, h = _blank(200)
    o[0][:], h[0][:] = -1.0, 0.0
    o[0][[10, 74]] = -5.0                    # g and g + 64: the same lane of two waves
    add("tie_g_and_g_plus_64", 200, o, h, (0 | 256, -5.0, 10, INF, INF, -1, INF, 200), F=0.0)
    o, h = _blank(300)
    o[0][:], h[0][:] = -1.0, 0.0
    o[0][[7, 263]] = -5.0                    # g and g + 256: one thread's two stride trips
    add("tie_g_and_g_plus_256", 300, o, h, (0 | 256, -5.0, 7, INF, INF, -1, INF, 300), F=0.0)
    o, h = _blank(100, both=True)
    for c in (0, 1):
        o[c][:], h[c][:] = -1.0, 0.0
        o[c][5] = -5.0                       # k = 5 of both centres: g = 5 and 105
    add("tie_k_in_both_centres", 100, o, h, (0 | 256, -5.0, 5, INF, INF, -1, INF, 200), F=0.0)
    # ... and among infeasible ones, a full (f, h) tie: dominating through I, the lower g is the new I
    o, h = _blank(400)
    o[0][[3, 300]] = -2.0
    add("full_f_h_tie", 400, o, h, (0, INF, -1, -2.0, 1.0, 3, 4.0, 2), I=(0.0, 4.0), h_max=16.0)
    # a candidate equal to (I.f, I.h): neither strict, the old I sorts first
    o, h = _blank(64)
    o[0][9] = -2.0
    add("candidate_equals_old_I", 64, o, h, (2, INF, -1, -2.0, 1.0, NEW_I_OLD, 1.0, 1), I=(-2.0, 1.0), h_max=1.0)
    # bestF.f == F.f: reported, no improvement; one ulp below: it replaces F
    o, h = _blank(1)
    o[0][0], h[0][0] = -3.0, 0.0
    add("bestF_equals_F", 1, o, h, (2, -3.0, 0, INF, INF, -1, INF, 1), F=-3.0)
    o, h = _blank(1)
    o[0][0], h[0][0] = below3, 0.0
    add("bestF_one_ulp_below_F", 1, o, h, (0 | 256, below3, 0, INF, INF, -1, INF, 1), F=-3.0)
    # only NaN objectives: all counted, nothing selected
    o, h = _blank(65, both=True)
    for c in (0, 1):
        o[c][:] = math.nan
        h[c][::2] = 0.0
    add("only_nan_objectives", 65, o, h, (2, INF, -1, 0.0, 2.0, NEW_I_OLD, 2.0, 130), F=0.0, I=(0.0, 2.0), h_max=2.0)
    # nothing evaluated
    o, h = _blank(129, both=True)
    add("everything_inf", 129, o, h, (2, INF, -1, INF, INF, -1, 7.0, 0), F=0.0, h_max=7.0)
    # h = 5e-324 is > 0: infeasible, however good its f (it becomes the new I, not the new F)
    o, h = _blank(2)
    o[0][:] = (-9.0, -1.0)
    h[0][:] = (5e-324, 0.0)
    add("subnormal_h_is_infeasible", 2, o, h, (0 | 256, -1.0, 1, -9.0, 5e-324, 0, INF, 2), F=0.0)
    # h one ulp below I.h with a worse f improves (h_new = that h, the old I leaves); one ulp above
    # counts for nothing, however good its f
    lo, hi = np.nextafter(2.0, -INF), np.nextafter(2.0, INF)
    o, h = _blank(2)
    o[0][:] = (0.0, -50.0)
    h[0][:] = (lo, hi)
    add("h_one_ulp_either_side_of_I", 2, o, h, (1, INF, -1, 0.0, lo, 0, lo, 2), I=(-1.0, 2.0), h_max=16.0)
    # the winners sit in the last slot, 2K - 1
    K = 6600
    o, h = _blank(K, both=True)
    for c in (0, 1):
        o[c][:], h[c][:] = -1.0, 0.0
    o[1][K - 1] = -7.0
    add("bestF_in_the_last_slot", K, o, h, (0 | 256, -7.0, 2 * K - 1, INF, INF, -1, INF, 2 * K), F=-1.0)
    o, h = _blank(K, both=True)
    for c in (0, 1):
        o[c][:], h[c][:] = -1.0, 3.0
    o[1][K - 1] = -7.0
    add("new_I_in_the_last_slot", K, o, h, (0, INF, -1, -7.0, 3.0, 2 * K - 1, 3.0, 2 * K), I=(-1.0, 3.0), h_max=3.0)
    # centre 0's whole poll was rejected (null arrays): the candidates of centre 1 keep g = K + k
    o, h = _blank(72, both=True)
    o[0] = h[0] = None
    o[1][3], h[1][3] = -4.0, 0.0
    add("centre_0_not_polled", 72, o, h, (0 | 256, -4.0, 75, -2.0, 1.0, NEW_I_OLD, 1.0, 1), F=-1.0, I=(-2.0, 1.0),
        h_max=1.0)
    return out


def select_cases():
    """The cases of prog_select_kernel's tests, the same list on every call: generated ones over every
    K x centres x (has_F, has_I) with quantised values (ties are the rule), four variants each that
    cycle through the unevaluated shares and the bias towards "improving"; then the hand-written ones."""
    if "select" not in _cache:
        rng = np.random.default_rng(20250216)
        shares = (0.0, 0.5, "most", 1.0)
        cases, q = [], 0
        for K in SELECT_KS:
            for centres in CENTRES:
                for has_F, has_I in ((1, 0), (0, 1), (1, 1)):
                    for v in range(4 if K < 3000 else 2):
                        share = shares[q % 4]
                        bias = bool(has_I) and (q // 4) % 2 == 0 and share in (0.0, 0.5)
                        c = _gen_case(rng, K, centres, has_F, has_I, share, bias)
                        c.update(name=f"gen{len(cases)}_K{K}_c{centres}_F{has_F}I{has_I}_{share}{'_b' if bias else ''}",
                                 centres=centres)
                        cases.append(c)
                        q += 1
                    q += 1   # (so that the shares do not line up with the loops above)
        for c in _hand_cases():
            c["centres"] = "both" if c["obj"][0] is not None and c["obj"][1] is not None else \
                "0" if c["obj"][0] is not None else "1"
            cases.append(c)
        _cache["select"] = cases
    return _cache["select"]


def diag_prog_select(pkg, ctx, obj, h, K, has_F, has_I, F_f, I_f, I_h, h_max, check=True):
    """mac_diag_prog_select (csrc/maxcover.hip; host only, not in maxcover.h): prog_select_kernel on the
    given arrays through the loop's own launch. Returns the record's eight fields (check=False: the
    return code alone)."""
    import ctypes
    L = pkg.load_library()
    dp, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    L.mac_diag_prog_select.argtypes = [ctypes.c_void_p, dp, dp, dp, dp, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, i64p]
    L.mac_diag_prog_select.restype = ctypes.c_int32
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (obj[0], h[0], obj[1], h[1])]
    assert not check or all(a is None or a.size >= K for a in arrs)
    ptrs = [None if a is None else a.ctypes.data_as(dp) for a in arrs]
    rec = np.zeros(8, dtype=np.int64)
    rc = L.mac_diag_prog_select(None if ctx is None else ctx._h, *ptrs, int(K), int(has_F), int(has_I), float(F_f),
                                float(I_f), float(I_h), float(h_max), rec.ctypes.data_as(i64p))
    if not check:
        return rc
    assert rc == 0, (rc, pkg.last_error() if hasattr(pkg, "last_error") else None)
    d = rec.view(np.float64)
    return (int(rec[0]), float(d[1]), int(rec[2]), float(d[3]), float(d[4]), int(rec[5]), float(d[6]), int(rec[7]))


# ---------------------------------------------------------------- the loop at N > 12

def rowwise_cons3(c3):
    """TDM_Constraints.create_cons3's callable with its loop over the UAVs vectorised (the same
    operations per UAV in the same order, so the same verdict: tests/test_prog_host.py compares them);
    carries c3's prev / d_lim / tan_half_fov. The host run at N = 600 calls it some 40,000 times."""
    prev, dl, t = c3.prev, c3.d_lim, c3.tan_half_fov
    N = prev.size // 3
    px, py, pz = prev[:N], prev[N:2 * N], prev[2 * N:] / t

    def cons3(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        dx, dy, dz = px - xx[:N], py - xx[N:2 * N], pz - xx[2 * N:] / t
        return not bool(np.any(np.sqrt(dx * dx + dy * dy + dz * dz) > dl))

    cons3.prev, cons3.d_lim, cons3.tan_half_fov = prev, dl, t
    return cons3


# The starts of test_larger_n_run_against_the_host_rule. "mixed": the first `above` radii start 0.25,
# 0.75, 0.5 above r_max = 30 tan 50 deg (less than one mesh step of 1), the others at `rest` below
# it: x0 is I, a poll that lowers the first ones gives a feasible F, two-centre polls follow.
# ell_max = 4: a basis of 2^4 = 16 > d_lim = 10 is rejected whole by cons3, an unsuccessful iteration
# with no launch (prog_select_kernel then gets null arrays for that centre).
LARGER_N = {
    22: dict(seed=22, above=1, rest=33.0, ell0=1, ell_max=4, n_iter=6),
    43: dict(seed=43, above=1, rest=33.0, ell0=1, ell_max=4, n_iter=6),
    512: dict(seed=512, above=2, rest=33.0, ell0=1, ell_max=4, n_iter=6),
    600: dict(seed=600, above=1, rest=33.0, ell0=1, ell_max=4, n_iter=6),
}
EXCESS = (0.25, 0.75, 0.5)
# "readme": the README's N = 512 run, every radius 0.2474 above its limit, so x0 is I and stays alone.
# The discs stand apart on a lattice of pitch 35 with their centres on multiples of 5 (midway between
# four points of the list) and the limit 13.0: a disc of radius 13.2474 covers 24 points there, 22 after
# a step of 1 in x or y and 16 with its radius lowered by 1. So at ell = 0 no trial point is at or below
# I.f, the 512 that lower one radius have h < I.h, all the same f and h equal up to the fold's rounding:
# an improving iteration decided by the ties alone, and h_max falls.
README_START = dict(seed=512, excess=0.2474, limit=13.0, ell0=0, ell_max=2, n_iter=4)


def larger_n_recipe(pkg, N, start="mixed", **over):
    """(rec, x0, r_max, kw): integer positions in [100, 700]^2 on the 800 x 800 list of grid_rec from
    SplitMix64(seed) (start "readme": README_START's lattice), the radii of the start, kw for TDM_STATIC_opt.mads (cons3 with d_lim = 10 around
    x0 is the caller's). ``over``: other values for the start's entries (choosing a recipe)."""
    p = dict(README_START if start == "readme" else LARGER_N[N], **over)
    rng = pkg.workloads.SplitMix64(p["seed"])
    r_max = np.full(N, 30.0 * TAN50)
    x = np.round(100.0 + rng.uniform(N) * 600.0)
    y = np.round(100.0 + rng.uniform(N) * 600.0)
    if start == "readme":
        iy, ix = np.divmod(np.arange(N), 23)
        assert N <= 23 * 23
        x, y = 15.0 + 35.0 * ix, 15.0 + 35.0 * iy
        r_max = np.full(N, float(p["limit"]))
        R = r_max + p["excess"]
    else:
        R = np.full(N, float(p["rest"]))
        R[:p["above"]] = r_max[:p["above"]] + np.array(EXCESS[:p["above"]])
    kw = dict(N_iter=p["n_iter"], ell0=p["ell0"], ell_max=p["ell_max"], seed=99)
    return grid_rec(pkg), np.concatenate([x, y, R]), r_max, kw
