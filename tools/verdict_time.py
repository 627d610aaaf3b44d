"""Constraint verdicts on config 5's MPC step (MAC_OPT_VERDICTS; k_cons.h cons_explain_gen_kernel):
FullSimulation.Simulation over the CA fire with cons_ext = [create_cons8(15.0)] and the reference's motion
values (cone_cos = -0.5, v_max = 2, a_max = 1; on from t = 3), from tools/mads_cons_time.py's "spaced"
start (every pair at least d_sep + 1 apart), with verdicts=True against verdicts=False.

Reported: ms per MPC step on and off (alternating runs, `--rounds` each, fresh context, fire and
simulation per run; medians and min-max), the split of the polled candidates by constraint that the
tally gives, and per poll the mask launch's time from the in-kernel stamps beside the explain launch's.
The explain launch takes no profile role and no stamps, so its time per poll is read two ways: the
step-time difference divided by the tallied polls (what a step pays, launch overhead included), and the
device time of the matrix kernel over one poll's candidates rebuilt on the host (`--explain-reps`
mac_cons_explain_f64 calls of K = 6N columns between two events, minus the same with K = 1: the upload
and the read-back are in both).
    python tools/verdict_time.py [--steps 3] [--warmup 2] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from tools.mads_cons_time import spaced_start  # noqa: E402

MOTION = dict(cone_cos=-0.5, v_max=2.0, a_max=1.0)
KINDS = ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")


def run(pkg, fire_kw, x0, seed, c8, steps, warmup, iters, verdicts, profile=False):
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, cons_ext=[c8],
                                            motion=MOTION, verdicts=verdicts)
        for _ in range(warmup):
            sim.step()
        torch.cuda.synchronize()
        if profile:
            ctx.profile(True)
            ctx.profile_read(reset=True)
        t0 = time.perf_counter()
        recs = [sim.step() for _ in range(steps)]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        kern = None
        if profile:
            kern = {k: {"ms": v, "launches": n} for k, (v, n) in ctx.profile_kernels().items() if n}
            ctx.profile_read(reset=True)
            ctx.profile(False)
        out = dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                   iterations=[int(r["iterations"]) for r in recs], f=[float(r["f"]) for r in recs],
                   rejected_polls=[int(r["rejected_polls"]) for r in recs],
                   candidates=int(sum(r["evaluations"] - 1 for r in recs)),
                   evaluated=int(sum(r["feasible_evaluations"] for r in recs)), kernels=kern,
                   outputs=[o.copy() for o in sim.outputs])
        if verdicts:
            out["polled_candidates"] = int(sum(r["polled_candidates"] for r in recs))
            out["rejected_any"] = int(sum(r["rejected_any"] for r in recs))
            out["rejected_by"] = {k: int(sum(r["rejected_by"][k] for r in recs)) for k in KINDS}
            out["polls"] = int(sum(r["iterations"] - r["rejected_polls"] for r in recs))
        return out


def explain_device_us(pkg, x, cons, motion, prev, d_lim, tan, reps):
    """Device time of cons_explain_kernel over one LTMADS-sized poll around x (K = 6N columns at step 2,
    every variable moved by at most 2), by events: K columns minus one column, per call."""
    rng = np.random.default_rng(5)
    n = x.size
    C = x[None, :] + rng.integers(-2, 3, (2 * n, n)).astype(np.float64)
    with pkg.Context(0) as ctx:
        def timed(M):
            ctx.cons_explain(M, cons=cons, motion=motion, prev=prev, d_lim=d_lim, tan_half_fov=tan)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(reps):
                ctx.cons_explain(M, cons=cons, motion=motion, prev=prev, d_lim=d_lim, tan_half_fov=tan)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps * 1e3
        full, one = timed(C), timed(C[:1])
    return dict(call_us_K=full, call_us_1=one, kernel_us_estimate=full - one, K=int(2 * n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mads-iters", type=int, default=100)
    ap.add_argument("--d-sep", type=float, default=15.0)
    ap.add_argument("--seed", type=int, default=20250216)
    ap.add_argument("--explain-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    wl = pkg.workloads
    cfg = wl.CONFIGS[5]
    rng = wl.SplitMix64(a.seed)
    fire_kw, x_bench = wl.config5_setup(rng, cfg["G"], cfg["N"], cfg["ignition"])
    c0 = cfg["G"] // 2 - cfg["ignition"] // 2 + 1
    x0 = spaced_start(x_bench, a.d_sep + 1.0, rng, (c0 - 1) * wl.PITCH, cfg["ignition"] * wl.PITCH)
    c8 = pkg.TDM_Constraints.create_cons8(a.d_sep)
    N = x0.size // 3
    args = (pkg, fire_kw, x0, a.seed, c8, a.steps, a.warmup, a.mads_iters)
    series = {"off": [], "on": []}
    last = {}
    for _ in range(a.rounds):   # alternating: drift hits both alike
        for kind in ("off", "on"):
            r = run(*args, kind == "on")
            series[kind].append(r["ms_per_step"])
            last[kind] = r
    prof = {kind: run(*args, kind == "on", profile=True) for kind in ("off", "on")}
    same = all(np.array_equal(p, q) for p, q in zip(last["on"]["outputs"], last["off"]["outputs"])) and \
        all(last["on"][k] == last["off"][k] for k in ("iterations", "f", "candidates", "evaluated", "rejected_polls"))
    on = last["on"]
    med = {k: float(np.median(v)) for k, v in series.items()}
    polls_per_step = on["polls"] / a.steps
    mk = {kind: prof[kind]["kernels"].get("cons_mask_gen_kernel", {"ms": 0.0, "launches": 0}) for kind in prof}
    # the explain kernel alone, on the last step's start (its MADS input) under the step's constraints
    tan = float(np.tan(100 / 180 * np.pi / 2))
    xin = on["outputs"][-2]
    dev = explain_device_us(pkg, xin, {"d_sep": a.d_sep},
                            dict(anchor=xin, vel=np.ones(2 * N), speed_prev=np.ones(N), **MOTION),
                            xin, np.full(N, 10.0), tan, a.explain_reps)
    out = {"tool": "verdict_time", "config": 5, "N": cfg["N"], "d_sep": a.d_sep, "motion": MOTION,
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "mads_iters": a.mads_iters,
           "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v} for k, v in series.items()},
           "on_over_off": med["on"] / med["off"],
           "outputs_and_stats_equal": bool(same),
           "kernel_launches_equal": {k: v["launches"] for k, v in prof["on"]["kernels"].items()} ==
                                    {k: v["launches"] for k, v in prof["off"]["kernels"].items()},
           "polls_per_step": polls_per_step,
           "explain_us_per_poll_from_step_difference": (med["on"] - med["off"]) * 1e3 / max(polls_per_step, 1),
           "explain_matrix_kernel": dev,
           "mask_us_per_poll": {kind: mk[kind]["ms"] / max(mk[kind]["launches"], 1) * 1e3 for kind in mk},
           "split": {"polled_candidates": on["polled_candidates"], "rejected_any": on["rejected_any"],
                     "evaluated": on["evaluated"], "rejected_by": on["rejected_by"],
                     "share_by": {k: on["rejected_by"][k] / max(on["polled_candidates"], 1) for k in KINDS},
                     "unevaluated_share": on["rejected_any"] / max(on["polled_candidates"], 1)},
           "on": {k: v for k, v in on.items() if k not in ("kernels", "outputs")},
           "off": {k: v for k, v in last["off"].items() if k not in ("kernels", "outputs")},
           "note": "split: over the candidates of the launched polls of the timed steps; a candidate counts "
                   "under every constraint that rejects it, so the shares by constraint add up to more than "
                   "unevaluated_share"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
