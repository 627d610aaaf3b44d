"""The native MADS driver's poll kinds on config 5's MPC step (FullSimulation.Simulation over the CA
fire, bench.py's config-5 set-up: 512 UAVs, 100 polls per step): poll_vars = "xyr" (every variable,
2 * 3N candidates per poll), "xy" (x and y only, 4N candidates, the radii held: MAC_POLL_XY) and
"auto" (per step: "xy" when every |R_i - r_max_i| <= 0.5). Per kind: ms per MPC step and per MADS run,
the objective reached and the area part of it, the evaluations (candidates that passed cons3), and
the kernels' times from the in-kernel stamps.

Every run is a fresh context, fire and simulation; the kinds alternate, `--rounds` times each;
wall-clock per step with the device synchronised, medians and min-max reported. The stamps come from
one more run of each kind (profiling on). All kinds start the first MPC step alike (the warmup step by
default); from the second on each kind continues from the circles and the list its own steps left,
so the timed steps' objectives compare trajectories, not single polls from one state.
    python tools/poll_vars_time.py [--steps 3] [--warmup 1] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

KINDS = ("xyr", "xy", "auto")


def run(pkg, fire_kw, x0, seed, kind, steps, warmup, iters, profile):
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, poll_vars=kind)
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
        N = x0.size // 3
        pen = [1e5 * float(np.sum(np.abs(o[2 * N:] - sim.r_max))) for o in sim.outputs[warmup:]]
        return dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                    poll_vars=[r.get("poll_vars", "xyr") for r in recs], iterations=[int(r["iterations"]) for r in recs],
                    f=[float(r["f"]) for r in recs], penalty=pen,
                    area=[p - float(r["f"]) for p, r in zip(pen, recs)],
                    successes=[int(r["successes"]) for r in recs],
                    candidates=[int(r["evaluations"]) - 1 for r in recs],
                    feasible_evaluations=[int(r["feasible_evaluations"]) for r in recs],
                    rejected_polls=[int(r["rejected_polls"]) for r in recs], kernels=kern)


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
    series = {k: [] for k in KINDS}
    mads = {k: [] for k in KINDS}
    last = {}
    for _ in range(a.rounds):   # alternating: drift hits all alike
        for kind in KINDS:
            r = run(pkg, fire_kw, x0, a.seed, kind, a.steps, a.warmup, a.mads_iters, False)
            series[kind].append(r["ms_per_step"])
            mads[kind].append(r["mads_ms_per_step"])
            last[kind] = r
    prof = {kind: run(pkg, fire_kw, x0, a.seed, kind, a.steps, a.warmup, a.mads_iters, True) for kind in KINDS}

    def stat(v):
        return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}

    out = {"tool": "poll_vars_time", "config": 5, "N": cfg["N"], "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "mads_iters": a.mads_iters,
           "start_radius_minus_r_max": float(x0[-1] - 30.0 * np.tan(100 / 180 * np.pi / 2)),
           "kinds": {kind: {"ms_per_step": stat(series[kind]), "mads_ms_per_step": stat(mads[kind]),
                            **{k: v for k, v in last[kind].items() if k not in ("kernels", "ms_per_step",
                                                                                "mads_ms_per_step")},
                            "kernels_ms": {k: v["ms"] for k, v in prof[kind]["kernels"].items()},
                            "kernels_launches": {k: v["launches"] for k, v in prof[kind]["kernels"].items()},
                            "kernels_us_per_launch": {k: v["ms"] / v["launches"] * 1e3
                                                      for k, v in prof[kind]["kernels"].items()}}
                     for kind in KINDS}}
    for kind in ("xy", "auto"):
        out[kind + "_over_xyr_ms"] = float(np.median(series[kind]) / np.median(series["xyr"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
