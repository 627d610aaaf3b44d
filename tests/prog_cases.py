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
        trial = []   # (f, h, centre, k, point) in (centre, k) order
        for c, xc in enumerate(centres):
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
                trial.append((obj(v), h, c, k, v))
        out["evaluated"] += len(trial)
        # 3: the best feasible trial point, the first in (centre, k) order among equals
        bestF = None
        for t in trial:
            if t[1] == 0.0 and (bestF is None or t[0] < bestF[0]):
                bestF = t
        improves = bestF is not None and (F is None or bestF[0] < F[1])
        # 4, 5
        dominating = improves
        improving = False
        if I is not None:
            for f, h, *_ in trial:
                if h > 0.0 and h <= I[2] and f <= I[1] and (h < I[2] or f < I[1]):
                    dominating = True
            if not dominating:
                for f, h, *_ in trial:
                    if h > 0.0 and h < I[2]:
                        improving = True
        # 7
        if improves:
            F = (bestF[4].copy(), bestF[0])
        if improving:
            h_new = max(h for f, h, *_ in trial if h > 0.0 and h < I[2])
        else:
            h_new = I[2] if I is not None else h_max
        newI = I if (I is not None and I[2] <= h_new) else None
        for f, h, c, k, v in trial:
            if h > 0.0 and h <= h_new:
                if newI is None or f < newI[1] or (f == newI[1] and h < newI[2]):
                    newI = (v.copy(), f, h)
        I = newI
        h_max = h_new
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
