"""The native MADS driver under a swarm constraint (mac_mads_run_cons) against the plain driver, on
config 5's MPC step (FullSimulation.Simulation over the CA fire, bench.py's config-5 set-up): ms per
MPC step with cons_ext = [create_cons8(d_sep)] and with none, the mask kernel's time per poll from
the in-kernel stamps, and the share of poll candidates left unevaluated.

Two starts: "bench" is bench.py's own (512 UAVs drawn uniformly over the ignition block: some pairs
start closer than d_sep, so f(x0) = +inf and a poll must separate all of them at once), "spaced"
re-draws every UAV that starts within d_sep + 1 of an earlier one (a feasible start: the case the
constraint is written for). Every run is a fresh context, fire and simulation; the on / off runs
alternate, `--rounds` times each; wall-clock per step with the device synchronised, medians and
min-max reported. The stamps come from one more run of each kind (profiling on).
    python tools/mads_cons_time.py [--steps 3] [--warmup 1] [--rounds 5] [--mads-iters 100] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def spaced_start(x0, d, rng, lo, span):
    """x0 with every UAV that lies within d of an earlier one re-drawn (same stream) until it does not."""
    x0 = x0.copy()
    N = x0.size // 3
    for i in range(1, N):
        while True:
            h = np.hypot(x0[:i] - x0[i], x0[N:N + i] - x0[N + i])
            if h.min() >= d:
                break
            x0[i] = np.round(lo + rng.uniform(1)[0] * span)
            x0[N + i] = np.round(lo + rng.uniform(1)[0] * span)
    return x0


def run(pkg, fire_kw, x0, seed, cons_ext, steps, warmup, iters, profile):
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, cons_ext=cons_ext)
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
        cands = sum(r["evaluations"] - 1 for r in recs)
        feas = sum(r["feasible_evaluations"] for r in recs)
        return dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                    iterations=[int(r["iterations"]) for r in recs], f=[float(r["f"]) for r in recs],
                    candidates=int(cands), evaluated=int(feas),
                    unevaluated_share=1.0 - feas / max(cands, 1), kernels=kern)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
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
    x_spaced = spaced_start(x_bench, a.d_sep + 1.0, rng, (c0 - 1) * wl.PITCH, cfg["ignition"] * wl.PITCH)
    c8 = pkg.TDM_Constraints.create_cons8(a.d_sep)
    out = {"tool": "mads_cons_time", "config": 5, "N": cfg["N"], "d_sep": a.d_sep, "steps": a.steps,
           "warmup": a.warmup, "rounds": a.rounds, "mads_iters": a.mads_iters, "starts": {}}
    for name, x0 in (("bench", x_bench), ("spaced", x_spaced)):
        N = x0.size // 3
        h = np.hypot(x0[:N, None] - x0[None, :N], x0[N:2 * N, None] - x0[None, N:2 * N])
        h[np.eye(N, dtype=bool)] = np.inf
        series = {"off": [], "on": []}
        last = {}
        for _ in range(a.rounds):   # alternating: drift hits both alike
            for kind, ce in (("off", ()), ("on", [c8])):
                r = run(pkg, fire_kw, x0, a.seed, ce, a.steps, a.warmup, a.mads_iters, False)
                series[kind].append(r["ms_per_step"])
                last[kind] = r
        prof = {kind: run(pkg, fire_kw, x0, a.seed, ce, a.steps, a.warmup, a.mads_iters, True)
                for kind, ce in (("off", ()), ("on", [c8]))}
        mk = prof["on"]["kernels"].get("cons_mask_gen_kernel", {"ms": 0.0, "launches": 0})
        out["starts"][name] = {
            "closest_pair": float(h.min()), "pairs_closer_than_d_sep": int((h < a.d_sep).sum() // 2),
            "ms_per_step": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}
                            for k, v in series.items()},
            "on_over_off": float(np.median(series["on"]) / np.median(series["off"])),
            "mask_us_per_poll": mk["ms"] / max(mk["launches"], 1) * 1e3, "mask_launches": mk["launches"],
            "off": {k: v for k, v in last["off"].items() if k != "kernels"},
            "on": {k: v for k, v in last["on"].items() if k != "kernels"},
            "kernels_us_per_launch": {kind: {k: v["ms"] / v["launches"] * 1e3 for k, v in prof[kind]["kernels"].items()}
                                      for kind in prof},
            "note": "unevaluated_share: poll candidates that fail cons3 or (on) the spacing; the "
                    "difference between on and off is the spacing's part on these iterates",
        }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
