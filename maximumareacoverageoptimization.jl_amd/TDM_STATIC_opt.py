"""Mirror of src/TDM_STATIC_opt.jl: the objective factory the solver calls and the MADS wrapper.

``createObjective(cells, N, r_max)`` (:82-100) packs ``cells.points_of_interest`` into the
device list ONCE per MPC step and returns ``AreaMaxObjective(x)`` with the reference closure
signature; ``AreaMaxObjective.batch(X)`` evaluates a whole poll (K x 3N) in one launch.

``optimize(input, obj, cons_ext, cons_prog, N_iter)`` (:118-222) stands in for DirectSearch's
``Optimize!`` (third-party, not vendored, version unpinned — SURVEY.md §8c): a granular MADS with
LTMADS-style integer poll directions (maximal basis, 2n trial points), extreme-barrier
constraints and a complete poll evaluated as one GPU batch. Its candidate sequence is NOT
DirectSearch's (parity unpinned); per-candidate objective values and the poll argmin are.
Returns ``(result, runtime_seconds)`` like the reference (:219-220).
"""
from __future__ import annotations

import time

import numpy as np

from ._lib import Context, InexactError, default_context, mesh_granularity
from .TDM_Constraints import merge_mac_cons, merge_mac_motion, merge_mac_prog, prog_h
from .workloads import SplitMix64, ltmads_basis

PENALTY = 1e5  # :97


def createObjective(cells, N: int, r_max, ctx: Context | None = None):
    """src/TDM_STATIC_opt.jl:82-100. ``r_max`` is read at call time (the reference closure
    captures the array by reference; src/FullSimulation.jl:64-76 mutates it between steps)."""
    ctx = ctx or default_context()
    pts = getattr(cells, "points_of_interest", cells)
    recs = np.asarray(pts, dtype=np.float64)
    if recs.ndim == 1:
        recs = recs.reshape(-1, 5)
    ctx.set_points_records(recs)

    def AreaMaxObjective(x) -> float:
        xx = np.asarray(x, dtype=np.float64)
        if xx.size % 3:
            raise InexactError(2, f"InexactError: Int64({xx.size}/3)")
        area_covered = ctx.area(xx)                     # :85-87
        violation = 0.0                                 # :89
        rm = np.asarray(r_max, dtype=np.float64)
        for i in range(N):                              # :90-93
            violation += abs(float(xx[i + 2 * N]) - float(rm[i]))
        return -area_covered + violation * PENALTY      # :97

    def batch(X) -> np.ndarray:
        Xa = np.asarray(X, dtype=np.float64)
        if Xa.ndim != 2 or Xa.shape[1] != 3 * N:
            raise ValueError("batch expects K x 3N")
        return ctx.objective_batch(Xa, np.asarray(r_max, dtype=np.float64), PENALTY)

    def poll(X, cons3=None, cons=None, motion=None):
        """(best_obj, best_idx, objectives) with cons3, the swarm constraints ``cons`` (a mac_cons
        mapping, TDM_Constraints.merge_mac_cons) and the target-motion constraints ``motion`` (a
        mac_motion mapping, merge_mac_motion) applied on the device."""
        Xa = np.asarray(X, dtype=np.float64)
        kw = {}
        if cons3 is not None and hasattr(cons3, "prev"):
            kw = dict(prev=cons3.prev, d_lim=cons3.d_lim, tan_half_fov=cons3.tan_half_fov)
        if cons is not None:
            kw["cons"] = cons
        if motion is not None:
            kw["motion"] = motion
        return ctx.poll_best(Xa, np.asarray(r_max, dtype=np.float64), PENALTY, want_all=True,
                             **kw)

    AreaMaxObjective.batch = batch
    AreaMaxObjective.poll = poll
    AreaMaxObjective.ctx = ctx
    AreaMaxObjective.N = N
    return AreaMaxObjective


class Status:
    def __init__(self):
        self.runtime_total = 0.0
        self.iteration = 0
        self.function_evaluations = 0
        # poll candidates passing cons3 (mac_mads_stats.feasible_evaluations: every candidate
        # without cons3) and polls where none does (a superset of mac_mads_stats.rejected_polls,
        # which counts the polls rejected by their diagonal steps alone)
        self.cons3_passed = 0
        self.cons3_empty_polls = 0
        self.successes = 0   # polls that moved the incumbent (mac_mads_stats.successes)
        # under progressive constraints (mads cons_prog=): the iterations by outcome, the polls
        # around both incumbents and the trial points evaluated (mac_mads_prog_stats)
        self.dominating = 0
        self.improving = 0
        self.unsuccessful = 0
        self.two_centre_polls = 0
        self.evaluated = 0
        self.optimization_status = "Unoptimized"


class MADSResult:
    """What the driver reads back: x (feasible best) or i (infeasible best), status."""

    def __init__(self):
        self.x = None
        self.i = None
        self.x_cost = np.inf
        # the infeasible incumbent's objective and h, and the barrier threshold (cons_prog= only)
        self.i_cost = np.inf
        self.i_h = None
        self.h_max = None
        # per iteration (outcome, F.x, F.f, I.x, I.f, I.h, h_max, centres polled) (cons_prog= only)
        self.history = []
        self.status = Status()


def polled_count(n: int, poll_vars: str = "xyr") -> int:
    """n_p, the variables a poll moves: all n = 3N ("xyr"), or x_0..x_{N-1}, y_0..y_{N-1} ("xy": the
    reference's CustomPoll, "directions only in the xy plane", src/TDM_STATIC_opt.jl:15-44)."""
    if poll_vars == "xyr":
        return n
    if poll_vars == "xy":
        return 2 * (n // 3)
    raise ValueError(f"poll_vars must be 'xyr' or 'xy', not {poll_vars!r}")


def poll_matrix(x: np.ndarray, B: np.ndarray) -> np.ndarray:
    """The 2 n_p candidates of a poll around x with the basis B (n_p x n_p): x + E B[:, k], then
    x - E B[:, k], E putting B's rows on the first n_p variables; the others (the radii of an
    xy-only poll) are x's doubles copied."""
    n_p = B.shape[0]
    if n_p == x.size:
        return np.concatenate([x[None, :] + B.T, x[None, :] - B.T], axis=0)
    X = np.repeat(x[None, :], 2 * n_p, axis=0)
    X[:n_p, :n_p] = x[None, :n_p] + B.T
    X[n_p:, :n_p] = x[None, :n_p] - B.T
    return X


def scaled_basis(B: np.ndarray, g) -> np.ndarray:
    """B with row v scaled by the granularity g[v] of polled variable v (one product per entry, the
    native driver's fl(g[v] * L); g None: B as it is)."""
    return B if g is None else g[:B.shape[0], None] * B


def mads(input, obj, cons_ext=(), N_iter: int = 100, ell0: int = 2, ell_max: int = 6,
         seed: int = 20250216, poll_vars: str = "xyr", granularity=None, cons_prog=(),
         h_max0=None) -> MADSResult:
    """Granular MADS, complete poll over D = [B, -B] (B an LTMADS-style integer basis whose
    entries are bounded by 2^ell), extreme barrier on cons_ext. Success: ell <- min(ell+1,
    ell_max) (larger steps); failure: ell <- ell-1; stop when ell < 0 (below the granularity
    1.0 of every variable, src/TDM_STATIC_opt.jl:131-137) or after N_iter iterations (:126).
    With a batched objective (``obj.poll``), cons3 and the constraints carrying ``mac_cons`` data
    (TDM_Constraints.create_cons8 / create_cons7) or ``mac_motion`` data (create_cons4 / create_cons5 /
    create_cons6) are applied on the device inside the poll; the
    iterates are the ones the same constraints give as plain host callables.
    ``poll_vars="xy"``: the basis is drawn over the n_p = 2N variables x, y (same stream, n := n_p)
    and the radii are held (MAC_POLL_XY, include/maxcover.h).
    ``granularity``: DirectSearch's SetGranularity (src/TDM_STATIC_opt.jl:131-137) per variable: None,
    a scalar, a pair (g_xy, g_r) or 3N values laid out as x; variable v steps by g[v] times the
    basis's integers (mac_mads_mesh, include/maxcover.h). None is 1.0 everywhere.
    ``cons_prog``: progressive constraints c_j(x) >= 0 (TDM_Constraints.create_cons1_progressive /
    create_cons_progressive, or plain callables), handled by the progressive barrier with the
    threshold ``h_max0`` (mads_prog below); empty: this loop as it is."""
    if len(cons_prog):
        return mads_prog(input, obj, cons_ext, cons_prog, h_max0, N_iter, ell0, ell_max, seed,
                         poll_vars, granularity)
    t0 = time.perf_counter()
    res = MADSResult()
    x = np.asarray(input, dtype=np.float64).copy()
    n = polled_count(x.size, poll_vars)
    g = mesh_granularity(granularity, x.size)
    rng = SplitMix64(seed)
    cons = list(cons_ext)

    def feasible(v) -> bool:
        return all(bool(c(v)) for c in cons)

    cons3 = next((c for c in cons if hasattr(c, "prev")), None)
    others = [c for c in cons if c is not cons3]
    # the swarm constraints that carry device data (create_cons8 / create_cons7) go to the poll as
    # one mac_cons; only the remaining plain callables are evaluated per candidate on the host
    dev_cons = dev_motion = None
    if hasattr(obj, "poll"):
        dev_cons, others = merge_mac_cons(others)
        dev_motion, others = merge_mac_motion(others)   # (cons4 / cons5 / cons6: one mac_motion)
    f = obj(x) if feasible(x) else np.inf
    res.status.function_evaluations += 1
    ell = ell0
    it = 0
    while it < N_iter and ell >= 0:
        it += 1
        B = scaled_basis(ltmads_basis(n, ell, rng).astype(np.float64), g)
        X = poll_matrix(x, B)
        n3 = sum(bool(cons3(v)) for v in X) if cons3 is not None else X.shape[0]
        res.status.cons3_passed += n3
        res.status.cons3_empty_polls += n3 == 0
        if hasattr(obj, "poll"):
            mask = np.array([all(bool(c(v)) for c in others) for v in X]) if others else None
            if mask is not None and not mask.any():
                bo, bi = np.inf, -1
            else:
                Xe = X if mask is None else X[mask]
                if dev_motion is not None:
                    bo, bi, _ = obj.poll(Xe, cons3, dev_cons, dev_motion)
                else:
                    bo, bi, _ = obj.poll(Xe, cons3) if dev_cons is None else obj.poll(Xe, cons3, dev_cons)
                if mask is not None and bi >= 0:
                    bi = int(np.flatnonzero(mask)[bi])
            res.status.function_evaluations += X.shape[0]
        else:
            bo, bi = np.inf, -1
            for k, v in enumerate(X):
                if not feasible(v):
                    continue
                fv = obj(v)
                res.status.function_evaluations += 1
                if fv < bo:
                    bo, bi = fv, k
        if bi >= 0 and bo < f:
            x, f = X[bi].copy(), bo
            ell = min(ell + 1, ell_max)
            res.status.successes += 1
        else:
            ell -= 1
    res.status.iteration = it
    res.status.runtime_total = time.perf_counter() - t0
    res.status.optimization_status = "MeshPrecisionLimit" if ell < 0 else "IterationLimit"
    if np.isfinite(f):
        res.x, res.x_cost = x, f
    else:
        res.i = x
    return res


def prog_select(F_f, I_f, I_h, h_max, cands):
    """Steps 3-7 of the progressive-barrier rule over the evaluated trial
    points ``cands`` = [(f, h, centre, k), ...] in (centre, k) order: F_f the feasible incumbent's
    objective or None, (I_f, I_h) the infeasible incumbent's or None. Returns (outcome, bestF,
    newI, h_new): outcome 'dominating' / 'improving' / 'unsuccessful'; bestF = (f, centre, k) when
    it replaces F, else None; newI = 'old', None or (f, h, centre, k). A trial point whose objective
    is NaN or +inf selects nothing (prog_select_kernel reads +inf as "not evaluated")."""
    cands = [t for t in cands if t[0] == t[0] and t[0] != np.inf]
    bestF = None
    for f, h, c, k in cands:
        if h == 0.0 and (bestF is None or f < bestF[0]):
            bestF = (f, c, k)
    improves = bestF is not None and (F_f is None or bestF[0] < F_f)
    inf_c = [t for t in cands if t[1] > 0.0]
    has_I = I_h is not None
    dominating = improves or (has_I and any(
        h <= I_h and f <= I_f and (h < I_h or f < I_f) for f, h, _, _ in inf_c))
    improving = not dominating and has_I and any(h < I_h for _, h, _, _ in inf_c)
    if improving:
        h_new = max(h for _, h, _, _ in inf_c if h < I_h)
    else:
        h_new = I_h if has_I else h_max
    newI = "old" if has_I and I_h <= h_new else None
    cur = (I_f, I_h) if newI == "old" else None
    for t in inf_c:
        f, h = t[0], t[1]
        if h <= h_new and (cur is None or f < cur[0] or (f == cur[0] and h < cur[1])):
            newI, cur = t, (f, h)
    outcome = "dominating" if dominating else "improving" if improving else "unsuccessful"
    return outcome, (bestF if improves else None), newI, h_new


def mads_prog(input, obj, cons_ext, cons_prog, h_max0=None, N_iter: int = 100, ell0: int = 2,
              ell_max: int = 6, seed: int = 20250216, poll_vars: str = "xyr",
              granularity=None) -> MADSResult:
    """``mads`` under progressive constraints: the progressive barrier of Audet & Dennis (2009) as
    DESIGN.md section 4 states it (the reference's AddProgressiveCollection,
    src/TDM_STATIC_opt.jl:142-159). h(x) = sum_j c_j(x)^2; a feasible incumbent F (h == 0) and an
    infeasible one I (0 < h <= h_max) are both polled with the iteration's one basis; trial points
    failing ``cons_ext``, with a NaN h or with h > h_max are dropped unevaluated. ``h_max0``: the
    initial threshold (None, negative or NaN: h(x0) when that is > 0, the reference's
    barrier_threshold^2, else +inf). With ``obj.poll`` and constraints that all carry ``mac_prog``
    data h comes from the device (Context.prog_h). Result: ``x`` = F.x, ``i`` = I.x (either may be
    None), ``x_cost`` / ``i_cost`` / ``i_h`` / ``h_max``."""
    t0 = time.perf_counter()
    res = MADSResult()
    st = res.status
    x0 = np.asarray(input, dtype=np.float64).copy()
    n = polled_count(x0.size, poll_vars)
    g = mesh_granularity(granularity, x0.size)
    rng = SplitMix64(seed)
    cons = list(cons_ext)
    progs = list(cons_prog)
    dev_prog = None
    if hasattr(obj, "poll"):
        dev_prog, plain = merge_mac_prog(progs, x0.size // 3)
        if plain:
            dev_prog = None

    def h_of(X):
        if dev_prog is not None:
            return np.asarray(obj.ctx.prog_h(X, dev_prog), dtype=np.float64)
        return np.array([prog_h([c(v) for c in progs]) for v in X], dtype=np.float64)

    def evaluate(X):
        if hasattr(obj, "poll"):
            return np.asarray(obj.poll(X)[2], dtype=np.float64)
        return np.array([obj(v) for v in X], dtype=np.float64)

    h0 = float(h_of(x0[None, :])[0])
    if h0 != h0:
        raise ValueError("cons_prog: h(x0) is NaN")
    given = h_max0 is not None and float(h_max0) >= 0.0
    h_max = float(h_max0) if given else (h0 if h0 > 0.0 else np.inf)
    if h0 > h_max:
        raise ValueError(f"cons_prog: h(x0) = {h0} > h_max0 = {h_max}")
    f0 = float(evaluate(x0[None, :])[0]) if all(bool(c(x0)) for c in cons) else np.inf
    st.function_evaluations += 1
    F = (x0, f0) if h0 == 0.0 else None
    I = None if h0 == 0.0 else (x0, f0, h0)
    ell = ell0
    it = 0
    while it < N_iter and ell >= 0:
        it += 1
        B = scaled_basis(ltmads_basis(n, ell, rng).astype(np.float64), g)
        centres = [p[0] for p in (F, I) if p is not None]
        st.two_centre_polls += len(centres) == 2
        cands, points = [], {}
        for c, xc in enumerate(centres):
            X = poll_matrix(xc, B)
            st.function_evaluations += X.shape[0]
            h = h_of(X)
            keep = np.array([all(bool(q(v)) for q in cons) for v in X], dtype=bool)
            keep &= ~(h != h) & ~(h > h_max)
            idx = np.flatnonzero(keep)
            if idx.size:
                fv = evaluate(X[idx])
                for k, f in zip(idx, fv):
                    cands.append((float(f), float(h[k]), c, int(k)))
                    points[(c, int(k))] = X[k]
        st.evaluated += len(cands)
        outcome, bestF, newI, h_new = prog_select(
            None if F is None else F[1], None if I is None else I[1],
            None if I is None else I[2], h_max, cands)
        if bestF is not None:
            F = (points[bestF[1:]].copy(), bestF[0])
        if newI is None:
            I = None
        elif newI != "old":
            I = (points[newI[2:]].copy(), newI[0], newI[1])
        h_max = h_new
        if outcome == "dominating":
            ell = min(ell + 1, ell_max)
            st.dominating += 1
            st.successes += 1
        elif outcome == "improving":
            st.improving += 1
        else:
            ell -= 1
            st.unsuccessful += 1
        res.history.append((outcome, None if F is None else F[0].copy(), None if F is None else F[1],
                            None if I is None else I[0].copy(), None if I is None else I[1],
                            None if I is None else I[2], h_max, len(centres)))
    st.iteration = it
    st.runtime_total = time.perf_counter() - t0
    st.optimization_status = "MeshPrecisionLimit" if ell < 0 else "IterationLimit"
    res.h_max = h_max
    if F is not None:
        res.x, res.x_cost = F
    if I is not None:
        res.i, res.i_cost, res.i_h = I
    return res


class PollStepper:
    """Host mirror of the native stepper (mac_mads_begin / _poll / _update, include/maxcover.h),
    driven by ``dist.mads_loop``: the poll sequence of ``mads`` (same stream, same update rule),
    of which this stepper evaluates only the shard [lo, hi) of every poll's 2n candidates, through
    ``poll_fn(X_shard) -> (best_obj, best_local_index)`` (index -1: nothing feasible). Every rank
    draws the whole basis, so all ranks stay at the same stream position. ``poll_vars`` and
    ``granularity``: as ``mads`` (n = n_p, the polled variables)."""

    def __init__(self, x0, f0: float, poll_fn, N_iter: int = 100, ell0: int = 2,
                 ell_max: int = 6, seed: int = 20250216, shard=None, poll_vars: str = "xyr",
                 granularity=None):
        self.x = np.asarray(x0, dtype=np.float64).copy()
        self.n = polled_count(self.x.size, poll_vars)
        self.g = mesh_granularity(granularity, self.x.size)
        self.f = float(f0)
        self.poll_fn = poll_fn
        self.N_iter, self.ell, self.ell_max = N_iter, ell0, ell_max
        self.rng = SplitMix64(seed)
        self.it = 0
        self.evals = 1
        self.lo, self.hi = (0, 2 * self.n) if shard is None else (int(shard[0]), int(shard[1]))
        self._X = None

    def poll(self):
        if self.it >= self.N_iter or self.ell < 0:
            return True, np.inf, -1
        self.it += 1
        B = scaled_basis(ltmads_basis(self.n, self.ell, self.rng).astype(np.float64), self.g)
        self._X = poll_matrix(self.x, B)
        Xs = self._X[self.lo:self.hi]
        if Xs.shape[0] == 0:
            return False, np.inf, -1
        bo, bi = self.poll_fn(Xs)
        return False, float(bo), (self.lo + int(bi) if bi >= 0 else -1)

    def update(self, best_obj: float, best_idx: int) -> None:
        self.evals += 2 * self.n
        if best_idx >= 0 and best_obj < self.f:
            self.x = self._X[best_idx].copy()
            self.f = float(best_obj)
            self.ell = min(self.ell + 1, self.ell_max)
        else:
            self.ell -= 1

    # speculation over failure branches (mac_mads_poll_ahead / mac_mads_advance)
    def _draws(self) -> int:
        n = self.n
        return n + n * (n - 1) // 2 + 2 * n   # ltmads_basis's stream values per iteration

    def _poll_matrix(self, ahead: int):
        rng = SplitMix64()
        with np.errstate(over="ignore"):
            rng.state = self.rng.state + np.uint64(ahead * self._draws()) * np.uint64(0x9E3779B97F4A7C15)
        B = scaled_basis(ltmads_basis(self.n, self.ell - ahead, rng).astype(np.float64), self.g)
        return poll_matrix(self.x, B)

    def poll_ahead(self, ahead: int):
        """(done, best_obj, best_idx, feasible): feasible is not tracked here (0)."""
        if self.it + ahead >= self.N_iter or self.ell - ahead < 0:
            return True, np.inf, -1, 0
        Xs = self._poll_matrix(ahead)[self.lo:self.hi]
        if Xs.shape[0] == 0:
            return False, np.inf, -1, 0
        bo, bi = self.poll_fn(Xs)
        return False, float(bo), (self.lo + int(bi) if bi >= 0 else -1), 0

    def advance(self, best_obj: float, best_idx: int) -> bool:
        X = self._poll_matrix(0)
        self.rng.next_u64(self._draws())   # the iteration's stream values
        self.it += 1
        self.evals += 2 * self.n
        if best_idx >= 0 and best_obj < self.f:
            self.x = X[best_idx].copy()
            self.f = float(best_obj)
            self.ell = min(self.ell + 1, self.ell_max)
            return True
        self.ell -= 1
        return False

    def result(self):
        return self.x.copy(), {"f": self.f, "iterations": self.it, "evaluations": self.evals,
                               "status": 0 if self.ell < 0 else 1}


# ---------------------------------------------------------------- the barrier's shard-partial record
# Plain-Python mirrors of csrc/prog_rule.h (DESIGN.md section 4 "Progressive barrier"): a record is the
# tuple of mac_prog_part's twelve fields in their order, the scalars are prog_select's (F_f, I_f, I_h,
# h_max) with None for an incumbent that does not exist.

PROG_TAG_DONE = 1 << 62
PROG_NEW_I_NONE, PROG_NEW_I_OLD = -1, -2


def _less2(f, g, f2, g2):
    return g >= 0 and (g2 < 0 or f < f2 or (f == f2 and g < g2))


def _less3(f, h, g, f2, h2, g2):
    return g >= 0 and (g2 < 0 or f < f2 or (f == f2 and (h < h2 or (h == h2 and g < g2))))


def prog_part_empty(tag: int = 0):
    inf = float("inf")
    return (int(tag), 0, inf, -1, 0, -1.0, inf, inf, -1, inf, inf, -1)


def prog_part(F_f, I_f, I_h, h_max, cands, tag: int = 0):
    """prog_part_fold over ``cands`` = [(f, h, g), ...] (g = centre K + k, any order): an objective of
    +inf is "not evaluated", a NaN one is counted and selects nothing."""
    tag, ev, bf, bg, dom, hb, kf, kh, kg, df, dh, dg = prog_part_empty(tag)
    has_I = I_h is not None
    thr = I_h if has_I else h_max
    for f, h, g in cands:
        f, h, g = float(f), float(h), int(g)
        if f == float("inf"):
            continue
        ev += 1
        if f != f:
            continue
        if h == 0.0:
            if _less2(f, g, bf, bg):
                bf, bg = f, g
        elif h > 0.0:
            if has_I:
                if h <= I_h and f <= I_f and (h < I_h or f < I_f):
                    dom = 1
                if h < I_h:
                    if h > hb:
                        hb = h
                    if _less3(f, h, g, df, dh, dg):
                        df, dh, dg = f, h, g
            if h <= thr and _less3(f, h, g, kf, kh, kg):
                kf, kh, kg = f, h, g
    return (tag, ev, bf, bg, dom, hb, kf, kh, kg, df, dh, dg)


def prog_merge(parts):
    """prog_part_merge over the records of one iteration (unequal tags: ValueError)."""
    parts = [tuple(p) for p in parts]
    if not parts:
        raise ValueError("prog_merge: no record")
    tag, ev, bf, bg, dom, hb, kf, kh, kg, df, dh, dg = parts[0]
    for p in parts[1:]:
        if p[0] != tag:
            raise ValueError(f"prog_merge: records of different iterations (tags {tag} and {p[0]})")
        ev += p[1]
        if _less2(p[2], p[3], bf, bg):
            bf, bg = p[2], p[3]
        dom |= p[4]
        hb = p[5] if p[5] > hb else hb
        if _less3(p[6], p[7], p[8], kf, kh, kg):
            kf, kh, kg = p[6:9]
        if _less3(p[9], p[10], p[11], df, dh, dg):
            df, dh, dg = p[9:12]
    return (tag, ev, bf, bg, dom, hb, kf, kh, kg, df, dh, dg)


def prog_finish(part, F_f, I_f, I_h, h_max):
    """prog_finish: ProgRec's eight fields (outcome | 256 when bestF replaces F, bestF_f, bestF_g,
    newI_f, newI_h, newI_g (-1: none, -2: the old one), h_new, evaluated) from the merged record."""
    _, ev, bf, bg, dom, hb, kf, kh, kg, df, dh, dg = part
    has_I = I_h is not None
    improves = bg >= 0 and (F_f is None or bf < F_f)
    dominating = improves or dom != 0
    improving = (not dominating) and has_I and hb > 0.0
    h_new = hb if improving else (I_h if has_I else h_max)
    nf, nh, ng = (df, dh, dg) if improving else (kf, kh, kg)
    if has_I and I_h <= h_new and not (ng >= 0 and (nf < I_f or (nf == I_f and nh < I_h))):
        nf, nh, ng = I_f, I_h, PROG_NEW_I_OLD
    code = (0 if dominating else 1 if improving else 2) | (256 if improves else 0)
    return (code, bf, bg, nf, nh, ng, h_new, ev)


def prog_chains(rec, has_I: bool) -> bool:
    """prog_chains: the iteration was unsuccessful and left I as it was (no I before and none after
    counts), so the poll one iteration ahead was the right one."""
    return (rec[0] & 255) == 2 and (rec[5] == PROG_NEW_I_OLD or (not has_I and rec[5] == PROG_NEW_I_NONE))


class ProgPollStepper:
    """Host mirror of the native prog stepper (mac_mads_begin_prog / _poll_prog / _advance_prog,
    include/maxcover.h), driven by ``dist.mads_prog_loop`` and ``dist.mads_prog_loop_speculative``:
    ``mads_prog``'s sequence (same stream, same rule), of which this stepper evaluates the shard
    [lo, hi) of every centre's poll as ``mads_prog`` evaluates a whole one. ``poll(ahead)`` ->
    (done, record) leaves the stepper as it is; ``advance(record)`` applies the iteration's merged
    record -> (outcome, chains). ``result()``: a MADSResult as ``mads_prog`` returns it."""

    def __init__(self, input, obj, cons_ext=(), cons_prog=(), h_max0=None, N_iter: int = 100,
                 ell0: int = 2, ell_max: int = 6, seed: int = 20250216, shard=None,
                 poll_vars: str = "xyr", granularity=None):
        x0 = np.asarray(input, dtype=np.float64).copy()
        self.n = polled_count(x0.size, poll_vars)
        self.g = mesh_granularity(granularity, x0.size)
        self.obj, self.cons, self.progs = obj, list(cons_ext), list(cons_prog)
        if not self.progs:
            raise ValueError("ProgPollStepper: cons_prog is empty (use PollStepper)")
        self.dev_prog = None
        if hasattr(obj, "poll"):
            self.dev_prog, plain = merge_mac_prog(self.progs, x0.size // 3)
            if plain:
                self.dev_prog = None
        self.N_iter, self.ell, self.ell_max = N_iter, ell0, ell_max
        self.rng = SplitMix64(seed)
        self.it = 0
        self.K = 2 * self.n
        self.lo, self.hi = (0, self.K) if shard is None else (int(shard[0]), int(shard[1]))
        self.shard = (self.lo, self.hi)
        self.res = MADSResult()
        h0 = float(self._h_of(x0[None, :])[0])
        if h0 != h0:
            raise ValueError("cons_prog: h(x0) is NaN")
        given = h_max0 is not None and float(h_max0) >= 0.0
        self.h_max = float(h_max0) if given else (h0 if h0 > 0.0 else np.inf)
        if h0 > self.h_max:
            raise ValueError(f"cons_prog: h(x0) = {h0} > h_max0 = {self.h_max}")
        f0 = float(self._evaluate(x0[None, :])[0]) if all(bool(c(x0)) for c in self.cons) else np.inf
        self.res.status.function_evaluations += 1
        self.F = (x0, f0) if h0 == 0.0 else None
        self.I = None if h0 == 0.0 else (x0, f0, h0)

    def _h_of(self, X):
        if self.dev_prog is not None:
            return np.asarray(self.obj.ctx.prog_h(X, self.dev_prog), dtype=np.float64)
        return np.array([prog_h([c(v) for c in self.progs]) for v in X], dtype=np.float64)

    def _evaluate(self, X):
        if hasattr(self.obj, "poll"):
            return np.asarray(self.obj.poll(X)[2], dtype=np.float64)
        return np.array([self.obj(v) for v in X], dtype=np.float64)

    def _draws(self) -> int:
        n = self.n
        return n + n * (n - 1) // 2 + 2 * n   # ltmads_basis's stream values per iteration

    def _basis(self, ahead: int):
        rng = SplitMix64()
        with np.errstate(over="ignore"):
            rng.state = self.rng.state + np.uint64(ahead * self._draws()) * np.uint64(0x9E3779B97F4A7C15)
        return scaled_basis(ltmads_basis(self.n, self.ell - ahead, rng).astype(np.float64), self.g)

    def _centres(self):
        return [p[0] for p in (self.F, self.I) if p is not None]

    def _scalars(self):
        return (None if self.F is None else self.F[1], None if self.I is None else self.I[1],
                None if self.I is None else self.I[2], self.h_max)

    def poll(self, ahead: int = 0):
        tag = self.it + ahead + 1
        if self.it + ahead >= self.N_iter or self.ell - ahead < 0:
            return True, prog_part_empty(tag | PROG_TAG_DONE)
        F_f, I_f, I_h, h_max = self._scalars()
        if ahead > 0 and I_h is not None:   # what an unsuccessful iteration leaves
            h_max = I_h
        B = self._basis(ahead)
        cands = []
        for c, xc in enumerate(self._centres()):
            X = poll_matrix(xc, B)[self.lo:self.hi]
            if X.shape[0] == 0:
                continue
            h = self._h_of(X)
            keep = np.array([all(bool(q(v)) for q in self.cons) for v in X], dtype=bool)
            keep &= ~(h != h) & ~(h > h_max)
            idx = np.flatnonzero(keep)
            if idx.size:
                fv = self._evaluate(X[idx])
                cands += [(float(f), float(h[k]), c * self.K + self.lo + int(k)) for k, f in zip(idx, fv)]
        return False, prog_part(F_f, I_f, I_h, h_max, cands, tag)

    def advance(self, part):
        part = tuple(part)
        if part[0] != self.it + 1:
            raise ValueError(f"ProgPollStepper.advance: the record's tag {part[0]} is not iteration {self.it + 1}")
        st = self.res.status
        centres = self._centres()
        B = self._basis(0)
        had_I = self.I is not None
        rec = prog_finish(part, *self._scalars())
        code, bestF_f, bestF_g, newI_f, newI_h, newI_g, h_new, evaluated = rec
        point = lambda g: poll_matrix(centres[g // self.K], B)[g % self.K].copy()   # noqa: E731
        newF = (point(bestF_g), bestF_f) if code & 256 else None
        newI = (point(newI_g), newI_f, newI_h) if newI_g >= 0 else None
        if newF is not None:
            self.F = newF
        if newI is not None:
            self.I = newI
        elif newI_g == PROG_NEW_I_NONE:
            self.I = None
        self.h_max = h_new
        st.two_centre_polls += len(centres) == 2
        st.function_evaluations += self.K * len(centres)
        st.evaluated += evaluated
        outcome = ("dominating", "improving", "unsuccessful")[code & 255]
        if outcome == "dominating":
            self.ell = min(self.ell + 1, self.ell_max)
            st.dominating += 1
            st.successes += 1
        elif outcome == "improving":
            st.improving += 1
        else:
            self.ell -= 1
            st.unsuccessful += 1
        F, I = self.F, self.I
        self.res.history.append((outcome, None if F is None else F[0].copy(), None if F is None else F[1],
                                 None if I is None else I[0].copy(), None if I is None else I[1],
                                 None if I is None else I[2], self.h_max, len(centres)))
        self.rng.next_u64(self._draws())   # the iteration's stream values
        self.it += 1
        return outcome, prog_chains(rec, had_I)

    def result(self) -> MADSResult:
        res, st = self.res, self.res.status
        st.iteration = self.it
        st.optimization_status = "MeshPrecisionLimit" if self.ell < 0 else "IterationLimit"
        res.h_max = self.h_max
        res.x, res.x_cost = self.F if self.F is not None else (None, np.inf)
        res.i, res.i_cost, res.i_h = self.I if self.I is not None else (None, np.inf, None)
        return res


def optimize(input, obj, cons_ext, cons_prog, N_iter: int):
    """src/TDM_STATIC_opt.jl:118-222: returns (p.x if feasible else p.i, runtime_total)."""
    p = mads(input, obj, cons_ext, N_iter, cons_prog=tuple(cons_prog or ()))
    result = p.i if p.x is None else p.x                # :165-169
    return result, p.status.runtime_total               # :219-220
