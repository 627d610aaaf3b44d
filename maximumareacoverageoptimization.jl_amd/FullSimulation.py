"""The hot-path part of src/FullSimulation.jl's MPC loop (run_simulation :23-278), on the GPU:
config 5 of BASELINE.json, a CA fire streamed into the point list every MPC step.

Per timestep t (:42-100):
  1. update_POI: new fire points appended to the device list (:50-52). The source is either the
     GPU cellular automaton (DynamicArea) or rows of a FirePoints table (src/CellFunctions.jl:59-79).
  2. drone_locs = the previous circles. rmvCoveredPOI deletes the entries they cover,
     order-preserving (:56-61).
  3. r_max update for UAVs at the 15 m altitude near the high-interest box (:64-76).
  4. cons3 around the previous circles (:78).
  5. The MADS input is drone_locs for t < 3, else the previous MADS output, unless it violates
     cons3 (:82-93).
  6. MADS (N_iter iterations) on the device: mac_mads_run, one complete LTMADS poll per
     iteration (:84-95). On P GPUs (``shard = (rank, P)``, config 5 "8 GPUs") every rank runs
     steps 1-5 itself — the fire CA is deterministic, so each GPU regenerates the same point
     list with no transfer — and polls its shard of every LTMADS poll (mac_mads_begin / _poll /
     _update); ``gather`` (dist.make_gather: a 16-B all-gather) combines the ranks' bests, so
     every rank holds the single-GPU iterates.
The trajectory stage (ALTRO, :107-251) is out of scope. The next step's circles are taken to be
the MADS output, i.e. perfect tracking, which the reference's trajectory stage aims at.
"""
from __future__ import annotations

import math
import time

import numpy as np

from ._lib import Context, mesh_granularity, percentage_covered
from .DynamicArea import DynamicArea

FOV = 100 / 180 * math.pi          # :735
h_max = 30.0                       # :737
N_iter = 100                       # :741
x_LB, x_UB, y_LB, y_UB = [2500], [3500], [1000], [2000]   # :751-754


def r_max_update(drone_locs: np.ndarray, r_max: np.ndarray, N: int, boxes=None) -> None:
    """:64-76 (t != 1): a UAV flying at ~15 m that is within h_max*tan(FOV/2) of the
    high-interest box keeps r_max = 15*tan(FOV/2); otherwise r_max = h_max*tan(FOV/2).
    ``boxes``: (x_LB, x_UB, y_LB, y_UB); None: the module's (:751-754)."""
    t2 = math.tan(FOV / 2)
    if boxes is None:
        boxes = (x_LB, x_UB, y_LB, y_UB)
    for i in range(N):
        if abs(15 - drone_locs[i + 2 * N] / t2) < 1:
            check = [(drone_locs[i] < xu + h_max * t2) and (drone_locs[i] > xl - h_max * t2) and
                     (drone_locs[i + N] < yu + h_max * t2) and (drone_locs[i + N] > yl - h_max * t2)
                     for xl, xu, yl, yu in zip(*boxes)]
            r_max[i] = 15 * t2 if any(check) else h_max * t2


def cons3_ok(prev: np.ndarray, x: np.ndarray, d_lim: np.ndarray) -> bool:
    """src/TDM_Constraints.jl:54-75 on the host (the pre-check of :88)."""
    N = x.size // 3
    t2 = math.tan(FOV / 2)
    for i in range(N):
        dx, dy = prev[i] - x[i], prev[N + i] - x[N + i]
        dz = prev[2 * N + i] / t2 - x[2 * N + i] / t2
        if math.sqrt(dx * dx + dy * dy + dz * dz) > d_lim[i]:
            return False
    return True


def auto_poll_vars(R, r_max, g_r=1.0) -> str:
    """The per-step choice of ``Simulation(poll_vars="auto")``: "xy" when every |R_i - r_max_i| <=
    g_r_i / 2 (0.5 on the unit mesh) at the MADS input — no step of a radius by its granularity
    ``g_r`` (a scalar or N values) then lowers the objective's 1e5 |R_i - r_max_i|
    (src/TDM_STATIC_opt.jl:92), the reference CustomPoll's "height constraint is already being
    satisfied" (:15-44) — else "xyr". Needs no GPU."""
    d = np.abs(np.asarray(R, dtype=np.float64) - np.asarray(r_max, dtype=np.float64))
    return "xy" if bool(np.all(d <= np.asarray(g_r, dtype=np.float64) / 2)) else "xyr"


def split_cons_ext(cons_ext):
    """The ``cons_ext`` slot of the reference's MADS call ([cons_ext, cons3], :86, :97) as the one
    mac_cons mapping the native driver takes (TDM_Constraints.merge_mac_cons; None: nothing on).
    ``cons1`` (always true) is dropped. A constraint the device cannot apply — a plain callable, or
    a second constraint of a kind already merged — raises ValueError naming it: the native driver
    generates its candidates on the device and calls no host function. The target-motion
    constraints (create_cons4 / create_cons5 / create_cons6) are merged into one mac_motion mapping
    (merge_mac_motion), returned under the key ``"motion"`` of the result. Needs no GPU."""
    from .TDM_Constraints import cons1, merge_mac_cons, merge_mac_motion
    if callable(cons_ext):
        cons_ext = [cons_ext]
    merged, plain = merge_mac_cons([c for c in (cons_ext or ()) if c is not cons1])
    motion, plain = merge_mac_motion(plain)
    if plain:
        names = ", ".join(getattr(c, "__name__", repr(c)) for c in plain)
        raise ValueError(f"cons_ext: {names} cannot run in the native MADS driver (no mac_cons data, "
                         "or a second constraint of a kind already given)")
    if motion is not None:
        merged = dict(merged or {}, motion=motion)
    return merged


def derive_motion(outputs, params, velocities=None, t=None):
    """The mac_motion mapping of MPC step ``t`` from the MADS outputs so far (None before two exist:
    "only activate after one iteration"): anchor = outputs[-1] (the reference's single_output);
    speed_prev[i] = the 3-D norm of UAV i's last target move outputs[-1] - outputs[-2], in the plain
    form sqrt(dx*dx + dy*dy + dz*dz); vel = the xy part of that move (perfect tracking), or what
    ``velocities(t)`` returns ([vx; vy], 2N). ``params``: cone_cos / v_max / a_max (missing or None:
    that constraint is off). Pure host arithmetic, the same on every rank."""
    if len(outputs) < 2:
        return None
    a = np.ascontiguousarray(np.asarray(outputs[-1], dtype=np.float64))
    b = np.asarray(outputs[-2], dtype=np.float64)
    N = a.size // 3
    d = a - b
    dx, dy, dz = d[:N], d[N:2 * N], d[2 * N:]
    m = {"anchor": a}
    if params.get("cone_cos") is not None:
        vel = np.concatenate([dx, dy]) if velocities is None else \
            np.asarray(velocities(t), dtype=np.float64).ravel()
        if vel.size != 2 * N:
            raise ValueError("velocities(t) must return 2N values [vx; vy]")
        m["vel"] = np.ascontiguousarray(vel)
        m["cone_cos"] = float(params["cone_cos"])
    if params.get("v_max") is not None:
        m["v_max"] = float(params["v_max"])
    if params.get("a_max") is not None:
        m["speed_prev"] = np.sqrt(dx * dx + dy * dy + dz * dz)
        m["a_max"] = float(params["a_max"])
    return m if len(m) > 1 else None


class Simulation:
    """The MPC loop as a stepper (one ``step()`` per timestep t = 1, 2, ...). Point source:
    ``fire`` (GPU CA: its initial points first, one CA step per MPC step), ``firepoints`` (table
    rows: rows 1..10 initially, then row t+10), or ``initial_points`` alone (static).
    ``attribution=True`` adds ``owned`` and ``exclusive`` (N doubles each, Context.area_by_disk of
    the step's MADS output on the step's list) to every record. ``cons_ext``: the swarm constraints
    MADS gets beside cons3 (TDM_Constraints.create_cons8 / create_cons7; split_cons_ext), applied on
    the device by every poll in all three modes (single, sharded, speculative).
    ``high_interest``: the high-interest boxes ``(x_LB, x_UB, y_LB, y_UB)`` (``True``: the module's,
    :751-754), set on the context before the first list upload (Context.set_regions) and left set
    afterwards: every fire point pushed strictly inside one gets the weight ``w_high`` (default
    (h_max*tan(FOV/2))^2*pi, src/CellFunctions.jl:44) on the device, the r_max rule reads the same
    boxes, and each record gains ``hi_total`` (points ever pushed inside the boxes), ``hi_uncovered``
    (those left in the list after the step's removal) and ``hi_percentage`` (:537-557). Every rank of
    a multi-GPU run sets the same regions; nothing is exchanged. None: no region call is made.
    ``poll_vars``: "xyr" (every variable, the default), "xy" (x and y only, the radii held:
    MAC_POLL_XY, the reference's CustomPoll, src/TDM_STATIC_opt.jl:15-44) or "auto" (per step, on the
    host after the r_max rule: auto_poll_vars); under "xy" and "auto" each record gains ``poll_vars``,
    what the step used (the default's records keep the keys they had).
    ``motion``: ``dict(cone_cos=, v_max=, a_max=)`` (the reference's -0.5, 2 and 1; a missing key: off)
    switches on cons4 / cons5 / cons6 (include/maxcover.h mac_motion) from t >= 3 on, around the
    previous MADS output (derive_motion); ``velocities``: a callable t -> [vx; vy] for cons4, None:
    the last target move (perfect tracking). Every rank derives the same arrays in all three modes;
    with ``motion=None`` the records and calls are what they were.
    ``granularity``: the MADS mesh of every step (None, a scalar, a pair (g_xy, g_r) or 3N values:
    Context.mads_run, mac_mads_mesh), in all three modes; "auto" then compares with g_r / 2. None:
    the calls as they were. ``mesh_keys``: True switches the context to keys in mesh units
    (Context.set_mesh_keys: the same results, every granularity at the unit mesh's packed keys); False
    (default) leaves the context's option as it is.
    ``cons_prog``: the progressive constraints MADS gets (the reference's cons_prog slot, :23, :86,
    :97), under the progressive barrier of Context.mads_run(prog=) with the first threshold
    ``h_max0`` (None: h at each step's MADS input). An entry is a constraint carrying ``mac_prog``
    data, or a factory called once with the simulation's own ``r_max`` array (the one the r_max rule
    updates): ``TDM_Constraints.create_cons1_progressive``, or
    ``functools.partial(create_cons_progressive, i)``. A callable without device data is refused
    (ValueError). With a shard the step runs dist.mads_prog_loop_speculative (more than one rank and
    ``speculate`` None or True) or dist.mads_prog_loop on Context.mads_prog_stepper, over a
    dist.RcclProgGather (the default on a cuda ``device``) or a dist.ProgGather; a given gather that is
    neither is refused (ValueError) before the context is used.
    Each record then gains ``h`` (of the step's output), ``has_feasible`` and the counts
    ``dominating`` / ``improving`` / ``unsuccessful``. ``penalty``: the objective's weight on
    sum |R_i - r_max_i| (src/TDM_STATIC_opt.jl:97), 1e5 as in the reference; 0 leaves the altitude to
    the progressive constraint alone.
    ``verdicts``: True switches on the native driver's tally of what rejected the candidates it polled
    (Context.set_verdicts) and reads and resets it once per step: each record gains ``rejected_by``
    (candidates per constraint, {"cons3": .., "cons8": .., "cons7": .., "cons4": .., "cons5": .., "cons6": ..};
    a candidate counts under every constraint that rejects it), ``rejected_any`` and
    ``polled_candidates`` (this rank's polls; the start points are not polled). The MADS outputs and the
    other fields are what they are without it; under ``cons_prog`` the driver ignores the option and the
    counts stay 0. False (default): the records and calls are what they were."""

    def __init__(self, ctx: Context, starting_circles, *, fire: DynamicArea | None = None,
                 firepoints=None, initial_points=None, N_iter: int = N_iter, d_lim=None,
                 r_max=None, seed: int = 20250216, ell0: int = 2, ell_max: int = 6,
                 shard=None, gather=None, speculate: bool | None = None, device=None,
                 attribution: bool = False, cons_ext=(), high_interest=None, w_high=None,
                 poll_vars: str = "xyr", motion=None, velocities=None, granularity=None,
                 cons_prog=(), h_max0=None, penalty: float = 1e5, mesh_keys: bool = False,
                 verdicts: bool = False):
        if poll_vars not in ("xyr", "xy", "auto"):
            raise ValueError(f"poll_vars must be 'xyr', 'xy' or 'auto', not {poll_vars!r}")
        self.poll_vars = poll_vars
        self.granularity = mesh_granularity(granularity, np.asarray(starting_circles).size)
        self.ctx = ctx
        self.mesh_keys = bool(mesh_keys)
        if self.mesh_keys:   # (Context.set_mesh_keys: read as each step's run begins)
            ctx.set_mesh_keys(True)
        self.verdicts = bool(verdicts)
        if self.verdicts:    # (Context.set_verdicts: read as each step's run begins; the tally starts at 0)
            ctx.set_verdicts(True)
            ctx.verdict_read(reset=True)
        self.high_interest = self._boxes(high_interest)
        if self.high_interest is None and w_high is not None:
            raise ValueError("w_high needs high_interest")
        self.cons = split_cons_ext(cons_ext)
        # motion constraints given as cons_ext callables keep their own (fixed) anchor
        self.cons_motion = self.cons.pop("motion", None) if self.cons else None
        self.cons = self.cons or None
        if motion is not None and self.cons_motion is not None:
            raise ValueError("motion= and a motion constraint in cons_ext share the one mac_motion")
        if motion is not None and set(motion) - {"cone_cos", "v_max", "a_max"}:
            raise ValueError("motion: the keys are cone_cos, v_max and a_max")
        self.motion = dict(motion) if motion is not None else None
        self.velocities = velocities
        # per-UAV attribution of each step's MADS output (one mac_area_by_disk_f64 call per step)
        self.attribution = bool(attribution)
        self.x_prev = np.asarray(starting_circles, dtype=np.float64).copy()
        self.N = N = self.x_prev.size // 3
        self.tan = math.tan(FOV / 2)
        self.d_lim = np.full(N, 10.0) if d_lim is None else np.asarray(d_lim, dtype=np.float64)
        self.r_max = (np.full(N, h_max * self.tan) if r_max is None
                      else np.asarray(r_max, dtype=np.float64).copy())
        self.penalty = float(penalty)
        self.h_max0 = h_max0
        self.cons_prog = self._cons_prog(cons_prog, shard, gather)
        self.fire, self.firepoints = fire, firepoints
        self.N_iter, self.seed, self.ell0, self.ell_max = N_iter, seed, ell0, ell_max
        self.shard = shard          # (rank, world) or None: the whole poll on this GPU
        # P GPUs: speculate over failure branches, rank j polling the poll after j failures
        # (gather: dist.SpecGather) — the default, since sharding one poll cannot shorten its
        # latency-bound chain — or shard every poll's candidates (speculate=False,
        # gather: dist.make_gather). With no gather given, the default one is made on `device`
        # (the collective's device: the rank's GPU under RCCL, "cpu" under gloo).
        multi = shard is not None and shard[1] > 1
        if speculate is None:
            from .dist import SpecGather
            # (a prog gather serves either loop: speculative unless speculate=False)
            speculate = multi and (gather is None or bool(self.cons_prog) or isinstance(gather, SpecGather))
        if multi and gather is None:
            from .dist import (ProgGather, RcclProgGather, RcclShardGather, RcclSpecGather, SpecGather,
                               make_gather)
            dev = device if device is not None else "cpu"
            if self.cons_prog:   # the 96-byte record, whichever loop
                gather = RcclProgGather(ctx, dev) if str(dev).startswith("cuda") else ProgGather(dev)
            elif str(dev).startswith("cuda"):   # libmaxcover's own RCCL communicator on ctx
                gather = RcclSpecGather(ctx, dev) if speculate else RcclShardGather(ctx, dev)
            else:
                gather = SpecGather(dev) if speculate else make_gather(dev)
        self.gather = gather
        self.speculate = bool(speculate)
        if self.high_interest is not None:
            self.w_high = (h_max * self.tan) ** 2 * math.pi if w_high is None else float(w_high)
            ctx.set_regions(*self.high_interest, w_high=self.w_high)
        if fire is not None:
            ctx.set_points_records(fire.initial_points())
        elif firepoints is not None:
            ctx.set_points_records(np.concatenate([np.asarray(r).reshape(-1, 5)
                                                   for r in firepoints[:10]] or [np.zeros((0, 5))]))
        else:
            ctx.set_points_records(np.asarray(initial_points, dtype=np.float64).reshape(-1, 5))
        self.t = 0
        self.outputs = []
        self.records = []

    def _cons_prog(self, cons_prog, shard, gather=None):
        """The progressive constraints bound to the simulation's r_max (an empty list: none)."""
        from .TDM_Constraints import merge_mac_prog
        if callable(cons_prog):
            cons_prog = [cons_prog]
        out = []
        for c in (cons_prog or ()):
            if not hasattr(c, "mac_prog"):
                try:
                    c = c(self.r_max)   # a factory: create_cons1_progressive, partial(create_cons_progressive, i)
                except Exception:
                    c = None
            if not hasattr(c, "mac_prog"):
                raise ValueError("cons_prog: a progressive constraint without device data (mac_prog) cannot "
                                 "run in the native MADS driver")
            out.append(c)
        if out and shard is not None and shard[1] > 1 and gather is not None:
            from .dist import ProgGather, RcclProgGather
            if not isinstance(gather, (ProgGather, RcclProgGather)):
                raise ValueError("cons_prog: a shard of more than one rank exchanges the barrier's 96-byte "
                                 "record: gather must be a dist.ProgGather or dist.RcclProgGather, not "
                                 f"{type(gather).__name__}")
        if out and merge_mac_prog(out, self.N)[1]:
            raise ValueError("cons_prog: the constraints do not fit one mac_prog (different limits, or "
                             "more than 32)")
        return out

    @staticmethod
    def _boxes(high_interest):
        """None, True (the module's boxes) or (x_LB, x_UB, y_LB, y_UB) as four equal-length lists."""
        if high_interest is None or high_interest is False:
            return None
        if high_interest is True:
            return (list(x_LB), list(x_UB), list(y_LB), list(y_UB))
        if len(high_interest) != 4:
            raise ValueError("high_interest must be (x_LB, x_UB, y_LB, y_UB)")
        b = tuple([float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64)).ravel()]
                  for q in high_interest)
        if len({len(q) for q in b}) != 1 or not b[0]:
            raise ValueError("high_interest: x_LB, x_UB, y_LB, y_UB must be non-empty and of equal length")
        return b

    def percentage_covered(self) -> float:
        """src/FullSimulation.jl:537-557, "Percentage of Area Covered": 100 - uncovered/total*100
        over the points strictly inside the boxes: total over every point ever pushed, uncovered
        over what is left in the list now. total = 0: NaN (Julia's 0/0)."""
        if self.high_interest is None:
            raise ValueError("percentage_covered needs high_interest")
        total = self.ctx.regions_ingested()[1]
        return percentage_covered(self.ctx.region_stats()["any_count"], total)

    def step(self) -> dict:
        ctx, N = self.ctx, self.N
        self.t += 1
        t = self.t
        t0 = time.perf_counter()
        added = 0
        if self.fire is not None:                                        # :50-52
            added = self.fire.fire.step(append_to=ctx)
        elif self.firepoints is not None and t != 1 and t + 10 - 1 < len(self.firepoints):
            row = np.asarray(self.firepoints[t + 10 - 1]).reshape(-1, 5)
            if row.shape[0]:
                ctx.append_points(row[:, 0], row[:, 1], row[:, 3])
                added = row.shape[0]
        t1 = time.perf_counter()
        drone_locs = self.x_prev.copy()                                  # :56-57
        kept = ctx.remove_covered(drone_locs)                            # :61
        t2 = time.perf_counter()
        if t != 1:
            r_max_update(drone_locs, self.r_max, N, self.high_interest)  # :64-76
        if t < 3:                                                        # :82-84
            single_input = drone_locs
        else:
            single_input = self.outputs[-1]
            if not cons3_ok(self.x_prev, single_input, self.d_lim):     # :88-90
                single_input = drone_locs
        kw = dict(prev=self.x_prev, d_lim=self.d_lim, tan_half_fov=self.tan, n_iter=self.N_iter,
                  ell0=self.ell0, ell_max=self.ell_max, seed=self.seed + t)
        if self.cons is not None:
            kw["cons"] = self.cons
        mo = self.cons_motion
        if self.motion is not None and t >= 3:
            mo = derive_motion(self.outputs, self.motion, self.velocities, t)
        if mo is not None:
            kw["motion"] = mo
        pvars = self.poll_vars
        if pvars == "auto":
            pvars = auto_poll_vars(single_input[2 * N:], self.r_max,
                                   1.0 if self.granularity is None else self.granularity[2 * N:])
        if pvars != "xyr":   # (the default: the calls as they were)
            kw["poll_vars"] = pvars
        if self.granularity is not None:
            kw["granularity"] = self.granularity
        if self.cons_prog:   # (merged per step: the limits are r_max as the rule above left it)
            from .TDM_Constraints import merge_mac_prog
            kw["prog"] = merge_mac_prog(self.cons_prog, N)[0]
            kw["h_max0"] = self.h_max0
        if self.cons_prog and self.shard is not None:   # (a shard of one rank: the stepper's loop, no exchange)
            from .dist import mads_prog_loop, mads_prog_loop_speculative, shard_range
            n_polled = single_input.size if pvars == "xyr" else 2 * N
            sh = None if self.speculate else shard_range(2 * n_polled, *self.shard)
            stepper = ctx.mads_prog_stepper(single_input, self.r_max, self.penalty, shard=sh, **kw)
            try:
                loop = mads_prog_loop_speculative if self.speculate else mads_prog_loop
                x_out, st = loop(stepper, self.gather)
            finally:
                stepper.close()
        elif self.shard is None or self.shard[1] == 1:
            x_out, st = ctx.mads_run(single_input, self.r_max, self.penalty, **kw)
        elif self.speculate:
            from .dist import mads_loop_speculative
            stepper = ctx.mads_stepper(single_input, self.r_max, self.penalty, **kw)
            try:
                x_out, st = mads_loop_speculative(stepper, self.gather)
            finally:
                stepper.close()
        else:
            from .dist import mads_loop, shard_range
            n_polled = single_input.size if pvars == "xyr" else 2 * N
            lo, hi = shard_range(2 * n_polled, *self.shard)
            stepper = ctx.mads_stepper(single_input, self.r_max, self.penalty, shard=(lo, hi), **kw)
            try:
                x_out, st = mads_loop(stepper, self.gather)
            finally:
                stepper.close()
        t3 = time.perf_counter()
        self.outputs.append(x_out)
        rec = dict(t=t, points=int(ctx.num_points), added=int(added), kept=int(kept.size),
                   f=st["f"], iterations=st["iterations"], evaluations=st["evaluations"],
                   feasible_evaluations=int(st.get("feasible_evaluations", 0)),
                   rejected_polls=int(st.get("rejected_polls", 0)),
                   successes=int(st.get("successes", 0)),
                   rounds=int(st.get("rounds", st["iterations"])),
                   useful_feasible_evaluations=int(st.get("useful_feasible_evaluations",
                                                          st.get("feasible_evaluations", 0))),
                   speculative_feasible_evaluations=int(st.get("speculative_feasible_evaluations",
                                                               st.get("feasible_evaluations", 0))),
                   slot_fallbacks=int(st.get("slot_fallbacks", 0)),
                   fire_s=t1 - t0, remove_s=t2 - t1, mads_s=t3 - t2, step_s=t3 - t0,
                   mads_host_s={k: float(st.get(k, 0.0)) for k in
                                ("host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")},
                   input=single_input)
        if self.poll_vars != "xyr":   # (the default's records are what they were)
            rec["poll_vars"] = pvars
        if self.cons_prog:
            from .TDM_Constraints import prog_h
            rec["h"] = prog_h([c(x_out) for c in self.cons_prog])
            rec["has_feasible"] = bool(st["has_feasible"])
            for k in ("dominating", "improving", "unsuccessful"):
                rec[k] = int(st[k])
        if self.verdicts:   # what rejected the step's polled candidates (read and reset once per step)
            v = ctx.verdict_read(reset=True)
            rec["rejected_by"] = v["rejected_by"]
            rec["rejected_any"] = v["rejected_any"]
            rec["polled_candidates"] = v["candidates"]
        if self.attribution:   # on the step's (post-removal) list
            rec["owned"], rec["exclusive"], _ = ctx.area_by_disk(x_out)
        if self.high_interest is not None:   # :537-557, on the step's (post-removal) list
            rec["hi_total"] = ctx.regions_ingested()[1]
            rec["hi_uncovered"] = ctx.region_stats()["any_count"]
            rec["hi_percentage"] = percentage_covered(rec["hi_uncovered"], rec["hi_total"])
        self.records.append(rec)
        self.x_prev = x_out                                              # perfect tracking
        return rec


def run_simulation(ctx: Context, starting_circles, Nt_sim: int, log=None, **kw):
    """run_simulation's optimisation side for Nt_sim steps: (records, MADS outputs)."""
    sim = Simulation(ctx, starting_circles, **kw)
    for _ in range(Nt_sim):
        rec = sim.step()
        if log:
            log(rec)
    return sim.records, sim.outputs
