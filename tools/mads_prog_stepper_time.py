"""The progressive barrier as a stepper against the host-stepped run, on tools/mads_prog_time.py's
protocol: config 5's MPC step (FullSimulation.Simulation over the CA fire, 512 UAVs, 100 iterations per
step) with cons_prog=[create_cons1_progressive] and penalty=0, three timed steps after a warm-up.
"run": Context.mads_run(prog=) (mac_mads_run_prog: prog_select_kernel, two passes, a 64-byte record).
"stepper": dist.mads_prog_loop on one whole-poll Context.mads_prog_stepper (Simulation(shard=(0, 1)):
mac_mads_poll_prog / mac_mads_advance_prog from Python, prog_part_kernel, one pass, a 96-byte record, no
exchange). The two enqueue the same launches except that last kernel; the stepper adds two ctypes calls
and a host merge per iteration.

Every run is a fresh context, fire and simulation; the variants alternate, `--rounds` times each;
wall-clock per step with the device synchronised, medians and min-max reported. prog_part_kernel's time
per launch comes from the stamps of its role (prog_select_kernel's, role 11) in one more, stepper-only
run. The outputs of the two variants must be equal. Recorded, not gated.
    python tools/mads_prog_stepper_time.py [--steps 3] [--warmup 1] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

VARIANTS = ("run", "stepper")


def run(pkg, fire_kw, x0, seed, variant, steps, warmup, iters, profile):
    kw = dict(cons_prog=[pkg.TDM_Constraints.create_cons1_progressive], penalty=0)
    if variant == "stepper":
        kw["shard"] = (0, 1)
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, **kw)
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
            kern = {k: {"ms": v, "launches": n, "us_per_launch": v / n * 1e3}
                    for k, (v, n) in ctx.profile_kernels().items() if n}
            ctx.profile_read(reset=True)
            ctx.profile(False)
        return dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                    host_s={k: sum(r["mads_host_s"][k] for r in recs) / steps * 1e3 for k in recs[0]["mads_host_s"]},
                    iterations=[int(r["iterations"]) for r in recs], f=[float(r["f"]) for r in recs],
                    h=[float(r["h"]) for r in recs], evaluations=[int(r["evaluations"]) for r in recs],
                    feasible_evaluations=[int(r["feasible_evaluations"]) for r in recs],
                    outcomes=[[r["dominating"], r["improving"], r["unsuccessful"]] for r in recs], kernels=kern,
                    outputs=[o.tobytes().hex() for o in sim.outputs[warmup:]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mads-iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=20250216)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    wl = pkg.workloads
    cfg = wl.CONFIGS[5]
    fire_kw, x0 = wl.config5_setup(wl.SplitMix64(a.seed), cfg["G"], cfg["N"], cfg["ignition"])
    series = {v: [] for v in VARIANTS}
    mads = {v: [] for v in VARIANTS}
    last = {}
    for _ in range(a.rounds):   # alternating: drift hits both alike
        for v in VARIANTS:
            r = run(pkg, fire_kw, x0, a.seed, v, a.steps, a.warmup, a.mads_iters, False)
            series[v].append(r["ms_per_step"])
            mads[v].append(r["mads_ms_per_step"])
            last[v] = r
    same = all(last["run"][k] == last["stepper"][k] for k in ("outputs", "f", "h", "iterations", "evaluations",
                                                              "feasible_evaluations", "outcomes"))
    prof = run(pkg, fire_kw, x0, a.seed, "stepper", a.steps, a.warmup, a.mads_iters, True)

    def stat(v):
        return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}

    drop = ("kernels", "ms_per_step", "mads_ms_per_step", "outputs")
    out = {"tool": "mads_prog_stepper_time", "config": 5, "N": cfg["N"], "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "mads_iters": a.mads_iters, "same_outputs": bool(same),
           "variants": {v: {"ms_per_step": stat(series[v]), "mads_ms_per_step": stat(mads[v]),
                            **{k: w for k, w in last[v].items() if k not in drop}} for v in VARIANTS},
           "stepper_kernels": prof["kernels"]}
    # (the stepper's last kernel is stamped under prog_select_kernel's role)
    out["prog_part_us_per_launch"] = prof["kernels"].get("prog_select_kernel", {}).get("us_per_launch")
    out["prog_h_us_per_launch"] = prof["kernels"].get("prog_h_kernel", {}).get("us_per_launch")
    out["stepper_over_run_ms"] = float(np.median(series["stepper"]) / np.median(series["run"]))
    lo, hi = min(series["run"]), max(series["run"])
    out["stepper_median_inside_run_spread"] = bool(lo <= np.median(series["stepper"]) <= hi)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("the stepper's outputs differ from the run's")


if __name__ == "__main__":
    main()
