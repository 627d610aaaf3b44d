"""The native MADS driver under a progressive constraint (mac_mads_run_prog) on config 5's MPC step
(FullSimulation.Simulation over the CA fire, bench.py's config-5 set-up: 512 UAVs, 100 iterations per
step, as tools/mads_granularity_time.py sets it up): a step with
cons_prog=[create_cons1_progressive] and penalty=0 ("prog") against the plain step ("plain": the
penalty 1e5 sum |R_i - r_max_i| and no progressive constraint, the pipelined loop). Per variant: ms
per MPC step and per MADS run, the objective, the evaluations; for "prog" also prog_h_kernel's and
prog_select_kernel's time per launch from the in-kernel stamps, the outcome counts per step, and the
final h and radii (their minimum, median and maximum, and sum max(R - r_max, 0)).

Every run is a fresh context, fire and simulation; the variants alternate, `--rounds` times each;
wall-clock per step with the device synchronised, medians and min-max reported. The stamps come from
one more run of each variant (profiling on). Recorded, not gated.
    python tools/mads_prog_time.py [--steps 3] [--warmup 1] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

VARIANTS = ("plain", "prog")


def run(pkg, fire_kw, x0, seed, variant, steps, warmup, iters, profile):
    kw = {}
    if variant == "prog":
        kw = dict(cons_prog=[pkg.TDM_Constraints.create_cons1_progressive], penalty=0)
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
        N = x0.size // 3
        R = sim.outputs[-1][2 * N:]
        out = dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                   iterations=[int(r["iterations"]) for r in recs], f=[float(r["f"]) for r in recs],
                   evaluations=[int(r["evaluations"]) for r in recs],
                   feasible_evaluations=[int(r["feasible_evaluations"]) for r in recs], kernels=kern,
                   final_radii={"min": float(R.min()), "median": float(np.median(R)), "max": float(R.max()),
                                "r_max_min": float(sim.r_max.min()), "r_max_max": float(sim.r_max.max()),
                                "excess": float(np.sum(np.maximum(R - sim.r_max, 0.0))),
                                "abs_gap": float(np.sum(np.abs(R - sim.r_max)))})
        if variant == "prog":
            out.update(h=[float(r["h"]) for r in recs], has_feasible=[bool(r["has_feasible"]) for r in recs],
                       dominating=[r["dominating"] for r in recs], improving=[r["improving"] for r in recs],
                       unsuccessful=[r["unsuccessful"] for r in recs])
        return out


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
    prof = {v: run(pkg, fire_kw, x0, a.seed, v, a.steps, a.warmup, a.mads_iters, True) for v in VARIANTS}

    def stat(v):
        return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}

    out = {"tool": "mads_prog_time", "config": 5, "N": cfg["N"], "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "mads_iters": a.mads_iters,
           "variants": {v: {"ms_per_step": stat(series[v]), "mads_ms_per_step": stat(mads[v]),
                            **{k: w for k, w in last[v].items() if k not in ("kernels", "ms_per_step",
                                                                             "mads_ms_per_step")},
                            "kernels": prof[v]["kernels"]} for v in VARIANTS}}
    pk = prof["prog"]["kernels"]
    out["prog_h_us_per_launch"] = pk.get("prog_h_kernel", {}).get("us_per_launch")
    out["prog_select_us_per_launch"] = pk.get("prog_select_kernel", {}).get("us_per_launch")
    out["prog_over_plain_ms"] = float(np.median(series["prog"]) / np.median(series["plain"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
