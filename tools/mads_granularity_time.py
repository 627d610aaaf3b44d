"""The native MADS driver's mesh (mac_mads_mesh: a granularity per variable) on config 5's MPC step
(FullSimulation.Simulation over the CA fire, bench.py's config-5 set-up: 512 UAVs, 100 polls per
step): granularity None (the unit mesh, the calls without a mesh), (1, 0.5), (1, 0.125), (1, 0.1) and
(0.5, 0.125) as (g_xy, g_r) under MAC_CHAIN_AUTO, and (1, 0.125) also under the forced five-launch
and the forced fused chain. Per variant: ms per MPC step and per MADS run, the objective reached with
its penalty and area parts, the evaluations (candidates that passed cons3), the polls rejected whole,
the kernels' times from the in-kernel stamps, and the fused chain's hint word 1 (disks that took one
position per candidate, Context.profile_fused).

Every run is a fresh context, fire and simulation; the variants alternate, `--rounds` times each;
wall-clock per step with the device synchronised, medians and min-max reported. The stamps come from
one more run of each variant (profiling on). All variants start the first MPC step alike; from the
second on each continues from the circles and the list its own steps left, so the timed steps'
objectives compare trajectories. The two forced runs decide where MAC_CHAIN_AUTO should send a
stepper whose granularity has a non-integer entry ("auto_route_for_fractional").
    python tools/mads_granularity_time.py [--steps 3] [--warmup 1] [--rounds 5] [--mads-iters 100] [--out FILE]

--mesh-keys: every row also with keys in mesh units (MAC_OPT_MESH_KEYS = MAC_KEYS_MESH, Context.set_mesh_keys;
rows NAME_mk), in the same alternating series. --parent-lib PATH: every value-key row also through another
build of the library (the parent commit's; rows NAME@parent), one child process per run (MAXCOVER_LIB is
read when the library loads), in the same series. The summary then compares, row by row, the mesh-key
runs with this build's value-key runs and the parent's ("mesh_keys": every run of the one below every run
of the other, the medians' ratio, and each row's ratio to the "none" row with its evaluation counts)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

# (name, granularity, chain)
VARIANTS = (("none", None, "auto"), ("1_0.5", (1.0, 0.5), "auto"), ("1_0.125", (1.0, 0.125), "auto"),
            ("1_0.1", (1.0, 0.1), "auto"), ("0.5_0.125", (0.5, 0.125), "auto"),
            ("1_0.125_five", (1.0, 0.125), "five"), ("1_0.125_fused", (1.0, 0.125), "fused"))
# --only none_fused: the unit mesh through the forced fused chain (the generated polls' fiw / fin2
# launches, which test the mesh pointer at run time): run once per library (MAXCOVER_LIB) for an A/B
# of the no-mesh path against another build
EXTRA = (("none_fused", None, "fused"),)


def run(pkg, fire_kw, x0, seed, gran, chain, steps, warmup, iters, profile, mesh_keys=False):
    with pkg.Context(0) as ctx:
        ctx.set_chain(chain)
        if mesh_keys:
            ctx.set_mesh_keys(True)
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        sim = pkg.FullSimulation.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, granularity=gran)
        for _ in range(warmup):
            sim.step()
        torch.cuda.synchronize()
        if profile:
            ctx.profile(True)
            ctx.profile_read(reset=True)
            ctx.profile_fused(reset=True)
        t0 = time.perf_counter()
        recs = [sim.step() for _ in range(steps)]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        kern = hint1 = None
        if profile:
            kern = {k: {"ms": v, "launches": n} for k, (v, n) in ctx.profile_kernels().items() if n}
            hint1 = ctx.profile_fused(reset=True)
            ctx.profile_read(reset=True)
            ctx.profile(False)
        N = x0.size // 3
        pen = [1e5 * float(np.sum(np.abs(o[2 * N:] - sim.r_max))) for o in sim.outputs[warmup:]]
        return dict(ms_per_step=ms, mads_ms_per_step=sum(r["mads_s"] for r in recs) / steps * 1e3,
                    iterations=[int(r["iterations"]) for r in recs],
                    f=[float(r["f"]) for r in recs], penalty=pen,
                    area=[p - float(r["f"]) for p, r in zip(pen, recs)],
                    successes=[int(r["successes"]) for r in recs],
                    feasible_evaluations=[int(r["feasible_evaluations"]) for r in recs],
                    rejected_polls=[int(r["rejected_polls"]) for r in recs], kernels=kern, hint_word_1=hint1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mads-iters", type=int, default=100)
    ap.add_argument("--seed", type=int, default=20250216)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one variant's timed runs alone (no profile run): its ms per step")
    ap.add_argument("--mesh-keys", action="store_true", help="every row also with keys in mesh units (NAME_mk)")
    ap.add_argument("--parent-lib", default=None, help="every value-key row also through this build of the library")
    a = ap.parse_args()
    pkg = ge.load_package()
    wl = pkg.workloads
    cfg = wl.CONFIGS[5]
    fire_kw, x0 = wl.config5_setup(wl.SplitMix64(a.seed), cfg["G"], cfg["N"], cfg["ignition"])
    if a.only:
        name, gran, chain = next(v for v in VARIANTS + EXTRA if v[0] == a.only)
        runs = [run(pkg, fire_kw, x0, a.seed, gran, chain, a.steps, a.warmup, a.mads_iters, False)
                for _ in range(a.rounds)]
        print(json.dumps({"tool": "mads_granularity_time", "only": name, "ms_per_step": [r["ms_per_step"] for r in runs],
                          "f": runs[-1]["f"], "feasible_evaluations": runs[-1]["feasible_evaluations"]}))
        return
    base_rows = VARIANTS
    rows = [(n, g, c, False) for n, g, c in base_rows]
    if a.mesh_keys:
        rows = [r for n, g, c in base_rows for r in ((n, g, c, False), (n + "_mk", g, c, True))]
    series = {v[0]: [] for v in rows}
    mads = {v[0]: [] for v in rows}
    parent = {n: [] for n, _, _ in base_rows} if a.parent_lib else {}
    parent_last = {}
    last = {}

    def parent_run(name):
        env = dict(os.environ, MAXCOVER_LIB=os.path.abspath(a.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--rounds", "1", "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--mads-iters", str(a.mads_iters), "--seed", str(a.seed)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, check=True)
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])

    for _ in range(a.rounds):   # alternating: drift hits all alike
        for name, gran, chain, mk in rows:
            r = run(pkg, fire_kw, x0, a.seed, gran, chain, a.steps, a.warmup, a.mads_iters, False, mk)
            series[name].append(r["ms_per_step"])
            mads[name].append(r["mads_ms_per_step"])
            last[name] = r
            print(f"{name}: {r['ms_per_step']:.2f} ms per step", file=sys.stderr, flush=True)
            if a.parent_lib and not mk:
                j = parent_run(name)
                parent[name].append(j["ms_per_step"][0])
                parent_last[name] = j
    prof = {name: run(pkg, fire_kw, x0, a.seed, gran, chain, a.steps, a.warmup, a.mads_iters, True, mk)
            for name, gran, chain, mk in rows}
    VARIANTS_ALL = [(n, g, c) for n, g, c, _ in rows]

    def stat(v):
        return {"median": float(np.median(v)), "min": min(v), "max": max(v), "runs": v}

    out = {"tool": "mads_granularity_time", "config": 5, "N": cfg["N"], "steps": a.steps, "warmup": a.warmup,
           "rounds": a.rounds, "mads_iters": a.mads_iters,
           "start_radius_minus_r_max": float(x0[-1] - 30.0 * np.tan(100 / 180 * np.pi / 2)),
           "variants": {name: {"granularity": gran, "chain": chain, "mesh_keys": name.endswith("_mk"),
                               "ms_per_step": stat(series[name]), "mads_ms_per_step": stat(mads[name]),
                               **{k: v for k, v in last[name].items() if k not in ("kernels", "ms_per_step",
                                                                                   "mads_ms_per_step", "hint_word_1")},
                               # the fused chain's reports the profiled run's enqueues read: how many,
                               # and over them the sum and the largest count of disks that took one
                               # position per candidate (a five-launch run writes none)
                               "hint_word_1": prof[name]["hint_word_1"],
                               "kernels_ms": {k: v["ms"] for k, v in prof[name]["kernels"].items()},
                               "kernels_launches": {k: v["launches"] for k, v in prof[name]["kernels"].items()},
                               "kernels_us_per_launch": {k: v["ms"] / v["launches"] * 1e3
                                                         for k, v in prof[name]["kernels"].items()}}
                        for name, gran, chain in VARIANTS_ALL}}
    base = float(np.median(series["none"]))
    for name, _, _ in VARIANTS_ALL[1:]:
        out[name + "_over_none_ms"] = float(np.median(series[name]) / base)
    if a.parent_lib:
        out["parent_lib_ms_per_step"] = {n: stat(v) for n, v in parent.items()}
        out["parent_lib_f"] = {n: j["f"] for n, j in parent_last.items()}
    if a.mesh_keys:
        mkc = {}
        for name, _, _ in base_rows:
            v, m = series[name], series[name + "_mk"]
            row = {"value_keys_median_ms": float(np.median(v)), "mesh_keys_median_ms": float(np.median(m)),
                   "mesh_over_value": float(np.median(m) / np.median(v)),
                   "every_mesh_run_below_every_value_run": max(m) < min(v),
                   "mesh_keys_over_none": float(np.median(m) / base),
                   "value_keys_over_none": float(np.median(v) / base),
                   "same_f": last[name]["f"] == last[name + "_mk"]["f"],
                   "feasible_evaluations": {"none": last["none"]["feasible_evaluations"],
                                            "value_keys": last[name]["feasible_evaluations"],
                                            "mesh_keys": last[name + "_mk"]["feasible_evaluations"]}}
            if a.parent_lib:
                pv = parent[name]
                row.update(parent_median_ms=float(np.median(pv)),
                           every_mesh_run_below_every_parent_run=max(m) < min(pv),
                           same_f_as_parent=parent_last[name]["f"] == last[name + "_mk"]["f"])
            mkc[name] = row
        out["mesh_keys"] = mkc
    five, fused = series["1_0.125_five"], series["1_0.125_fused"]
    # the faster forced chain at g_r = 0.125; "undecided" when the runs' ranges overlap
    if max(five) < min(fused):
        route = "five"
    elif max(fused) < min(five):
        route = "fused"
    else:
        route = "undecided"
    out["auto_route_for_fractional"] = {"decision": route, "five_median_ms": float(np.median(five)),
                                        "fused_median_ms": float(np.median(fused)),
                                        "auto_median_ms": float(np.median(series["1_0.125"])),
                                        "rule": "every run of one forced chain below every run of the other"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
