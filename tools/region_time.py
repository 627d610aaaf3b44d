"""High-interest regions (mac_set_regions / mac_region_stats_f64 / the ingest launch) timed on the
device; writes profiles/regions.json.

  stats   Context.region_stats on the config-4 grid (4096^2 = 16.8M entries): the reference's 1 km^2
          box (src/FullSimulation.jl:751-754) and a whole-domain box, each without disks and with 512,
          against the only route without the call: get_points (and covered_flags) plus the numpy mask.
  ingest  set_points of that grid, and an append of `--append` entries to config 5's initial list
          (512^2 entries), with regions on and off, alternating.
  step    config 5's MPC step (FullSimulation.Simulation over the CA fire, bench.py's set-up) with a
          box over the burning block and the reference's w_high against the same step without regions,
          alternating; the launch roles of the polls from the in-kernel stamps (which shared-entry
          pass ran) from one more run of each kind.

Wall-clock with the device synchronised; medians and min-max over `--rounds` runs.
    python tools/region_time.py [--rounds 5] [--steps 2] [--warmup 1] [--mads-iters 100] [--only stats,ingest,step] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def timed(f, rounds):
    out = []
    res = None
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out, res


def summary(ms):
    return dict(ms=ms, median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def stats_part(pkg, rounds):
    wl = pkg.workloads
    lib = pkg._lib
    x, y, w = wl.grid_points(4096)
    side = 4096 * wl.PITCH
    disks = wl.uniform_disks(512, 4096, wl.SplitMix64(3))
    cases = {"reference box (1 km^2)": ([2500.0], [3500.0], [1000.0], [2000.0]),
             "whole domain": ([-1.0], [side + 1.0], [-1.0], [side + 1.0])}
    out = {"entries": int(x.size)}
    with pkg.Context(0) as ctx:
        ctx.set_points(x, y, w)
        for name, box in cases.items():
            ctx.set_regions(*box)
            for label, circ in (("no disks", None), ("512 disks", disks)):
                ctx.region_stats(circ)   # (buffers allocated)
                ms, got = timed(lambda: ctx.region_stats(circ), rounds)

                def host_route():
                    gx, gy, gw = ctx.get_points()
                    m = lib.high_interest_mask(gx, gy, box)
                    r = dict(any_count=int(m.sum()), any_weight=float(gw[m].sum()))
                    if circ is not None:
                        c = ctx.covered_flags(circ) & m
                        r.update(covered_count=int(c.sum()), covered_weight=float(gw[c].sum()))
                    return r

                hms, want = timed(host_route, max(2, rounds // 2))
                for k, v in want.items():
                    assert got[k] == v, (name, label, k, got[k], v)
                out[f"{name}, {label}"] = dict(region_stats=summary(ms), get_points_numpy=summary(hms),
                                               speedup=float(np.median(hms) / np.median(ms)),
                                               any_count=got["any_count"], covered_count=got["covered_count"])
    return out


def ingest_part(pkg, rounds, m_append):
    wl = pkg.workloads
    x, y, w = wl.grid_points(4096)
    box = ([2500.0], [3500.0], [1000.0], [2000.0])
    rng = wl.SplitMix64(17)
    c0 = (2048 - 256) * wl.PITCH
    bx, by, bw = wl.grid_points(512)
    bx, by = bx + c0, by + c0
    ax = c0 + rng.uniform(m_append) * 512 * wl.PITCH
    ay = c0 + rng.uniform(m_append) * 512 * wl.PITCH
    aw = np.full(m_append, 25.0)
    abox = ([c0 + 500.0], [c0 + 1500.0], [c0 + 500.0], [c0 + 1500.0])
    res = {k: {"on": [], "off": []} for k in ("set_points 16.8M", f"append {m_append} to 262144")}
    with pkg.Context(0) as ctx:
        ctx.set_points(x, y, w)
        for _ in range(rounds):
            for mode in ("off", "on"):
                ctx.set_regions(*box, w_high=7854.0) if mode == "on" else ctx.clear_regions()
                ms, _ = timed(lambda: ctx.set_points(x, y, w), 1)
                res["set_points 16.8M"][mode] += ms
        ctx.clear_regions()
        for _ in range(rounds):
            for mode in ("off", "on"):
                ctx.clear_regions()
                ctx.set_points(bx, by, bw)
                if mode == "on":
                    ctx.set_regions(*abox, w_high=7854.0)
                ms, _ = timed(lambda: ctx.append_points(ax, ay, aw), 1)
                res[f"append {m_append} to 262144"][mode] += ms
    return {k: dict(on=summary(v["on"]), off=summary(v["off"]),
                    ratio=float(np.median(v["on"]) / np.median(v["off"]))) for k, v in res.items()}


def step_run(pkg, fire_kw, x0, seed, box, steps, warmup, iters, profile):
    FS = pkg.FullSimulation
    with pkg.Context(0) as ctx:
        D = pkg.DynamicArea.DynamicArea(**fire_kw, seed=seed, device=0)
        kw = dict(high_interest=box) if box is not None else {}
        sim = FS.Simulation(ctx, x0, fire=D, N_iter=iters, seed=seed, **kw)
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
        hi = {k: recs[-1][k] for k in ("hi_total", "hi_uncovered", "hi_percentage") if k in recs[-1]}
        D.close()
    return ms, kern, hi, [r["mads_s"] * 1e3 for r in recs]


def step_part(pkg, rounds, steps, warmup, iters, seed=20250216):
    wl = pkg.workloads
    cfg = wl.CONFIGS[5]
    fire_kw, x0 = wl.config5_setup(wl.SplitMix64(seed), cfg["G"], cfg["N"], cfg["ignition"])
    lo, hi = fire_kw["x_start1"] - wl.PITCH, fire_kw["x_start2"]
    q = (hi - lo) / 4   # the middle of the burning block, a quarter of its area
    box = ([lo + q], [hi - q], [lo + q], [hi - q])
    ms = {"on": [], "off": []}
    mads = {"on": [], "off": []}
    hi_rec = None
    for _ in range(rounds):
        for mode in ("off", "on"):
            t, _, h, m = step_run(pkg, fire_kw, x0, seed, box if mode == "on" else None, steps, warmup, iters, False)
            ms[mode].append(t)
            mads[mode] += m
            hi_rec = h or hi_rec
    kern = {mode: step_run(pkg, fire_kw, x0, seed, box if mode == "on" else None, steps, warmup, iters, True)[1]
            for mode in ("off", "on")}
    return dict(box=box, w_high=(30.0 * math.tan(100 / 180 * math.pi / 2)) ** 2 * math.pi, mads_iters=iters,
                steps=steps, ms_per_step_on=summary(ms["on"]), ms_per_step_off=summary(ms["off"]),
                ratio=float(np.median(ms["on"]) / np.median(ms["off"])),
                mads_ms_on=summary(mads["on"]), mads_ms_off=summary(mads["off"]),
                kernels=kern, last_record=hi_rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mads-iters", type=int, default=100)
    ap.add_argument("--append", type=int, default=100000)
    ap.add_argument("--only", default="stats,ingest,step")
    ap.add_argument("--out", default=os.path.join(ge.ROOT, "profiles", "regions.json"))
    a = ap.parse_args()
    pkg = ge.load_package()
    out = {"tool": "tools/region_time.py", "version": pkg.version(), "rounds": a.rounds}
    if os.path.exists(a.out):   # (parts measured by an earlier call are kept)
        with open(a.out) as f:
            out = {**json.load(f), **out}
    only = a.only.split(",")
    if "stats" in only:
        out["stats"] = stats_part(pkg, a.rounds)
    if "ingest" in only:
        out["ingest"] = ingest_part(pkg, a.rounds, a.append)
    if "step" in only:
        out["step"] = step_part(pkg, a.rounds, a.steps, a.warmup, a.mads_iters)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
