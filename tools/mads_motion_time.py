"""The native MADS driver under the target-motion constraints (mac_mads_run_motion: cons4 / cons5 /
cons6, include/maxcover.h mac_motion) on config 5's MPC step (FullSimulation.Simulation over the CA
fire, bench.py's config-5 set-up with tools/mads_cons_time.py's "spaced" start): ms per MPC step
with motion= set to the reference's values (cone_cos -0.5, v_max 2, a_max 1), with nothing, and with
cons8 alone; the mask kernel's time per poll from the in-kernel stamps; the share of poll candidates
left unevaluated.

The motion constraints switch on at t = 3 (two targets exist), so the first two steps are warm-up
and the timed steps start there. Every run is a fresh context, fire and simulation; the three kinds
alternate, `--rounds` times each; wall-clock per step with the device synchronised, medians and
min-max reported. The stamps come from one more run of each kind (profiling on).
    python tools/mads_motion_time.py [--steps 3] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402
from mads_cons_time import spaced_start  # noqa: E402

REFERENCE = dict(cone_cos=-0.5, v_max=2.0, a_max=1.0)   # src/TDM_Constraints.jl:78-138
WARMUP = 2                                              # t = 1, 2: no motion constraint yet


def run(pkg, fire_kw, x0, seed, kw, steps, iters, profile):
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, **kw)
        for _ in range(WARMUP):
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
        cands = sum(r["evaluations"] - 1 for r in recs)
        feas = sum(r["feasible_evaluations"] for r in recs)
        return dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                    iterations=[int(r["iterations"]) for r in recs], f=[float(r["f"]) for r in recs],
                    candidates=int(cands), evaluated=int(feas),
                    unevaluated_share=1.0 - feas / max(cands, 1), kernels=kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mads-iters", type=int, default=100)
    ap.add_argument("--d-sep", type=float, default=15.0)
    ap.add_argument("--seed", type=int, default=20250216)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    wl = pkg.workloads
    cfg = wl.CONFIGS[5]
    rng = wl.SplitMix64(a.seed)
    fire_kw, x_bench = wl.config5_setup(rng, cfg["G"], cfg["N"], cfg["ignition"])
    c0 = cfg["G"] // 2 - cfg["ignition"] // 2 + 1
    x0 = spaced_start(x_bench, a.d_sep + 1.0, rng, (c0 - 1) * wl.PITCH, cfg["ignition"] * wl.PITCH)
    kinds = (("off", {}), ("cons8", {"cons_ext": [pkg.TDM_Constraints.create_cons8(a.d_sep)]}),
             ("motion", {"motion": REFERENCE}))
    series = {k: [] for k, _ in kinds}
    last = {}
    for _ in range(a.rounds):   # alternating: drift hits all alike
        for kind, kw in kinds:
            r = run(pkg, fire_kw, x0, a.seed, kw, a.steps, a.mads_iters, False)
            series[kind].append(r["ms_per_step"])
            last[kind] = r
    prof = {kind: run(pkg, fire_kw, x0, a.seed, kw, a.steps, a.mads_iters, True) for kind, kw in kinds}

    def mask(kind):
        mk = prof[kind]["kernels"].get("cons_mask_gen_kernel", {"ms": 0.0, "launches": 0})
        return {"us_per_poll": mk["ms"] / max(mk["launches"], 1) * 1e3, "launches": mk["launches"]}

    med = {k: float(np.median(v)) for k, v in series.items()}
    out = {"tool": "mads_motion_time", "config": 5, "N": cfg["N"], "motion": REFERENCE, "d_sep": a.d_sep,
           "steps": a.steps, "warmup": WARMUP, "rounds": a.rounds, "mads_iters": a.mads_iters,
           "ms_per_step": {k: {"median": med[k], "min": min(v), "max": max(v), "runs": v}
                           for k, v in series.items()},
           "motion_over_off": med["motion"] / med["off"], "motion_over_cons8": med["motion"] / med["cons8"],
           "cons8_over_off": med["cons8"] / med["off"],
           "mask": {k: mask(k) for k in ("cons8", "motion")},
           "runs": {k: {q: v for q, v in last[k].items() if q != "kernels"} for k in last},
           "kernels_us_per_launch": {kind: {k: v["ms"] / v["launches"] * 1e3
                                            for k, v in prof[kind]["kernels"].items()} for kind in prof},
           "note": "unevaluated_share: poll candidates that fail cons3 or the kind's constraints; mask: "
                   "the stamp role cons_mask_gen_kernel covers the motion kernels as well"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
