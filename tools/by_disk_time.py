"""Per-UAV attribution (mac_area_by_disk_f64, by_disk_kernel) against its yardstick, the
single-candidate closure call (mac_area_f64, closure_kernel), on the same candidate: the
incumbent of config 4 (N = 512, 16.8M entries), column 0 of the candidate matrix.

Per-call wall time of Context.area_by_disk and Context.area (each call ends with its result on the
host), in alternating blocks after a warm-up of both; then, in a pass of its own, the two kernels'
spans from the in-kernel stamps (MAC_OPT_PROFILE). Asserts sum(owned) == area == Context.area bit
for bit and prints one JSON line.
    python tools/by_disk_time.py [--config 4] [--rounds 7] [--calls 1000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def block(fn, c, calls):
    t = time.perf_counter()
    for _ in range(calls):
        fn(c)
    return (time.perf_counter() - t) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    x, y, w, C, _ = pkg.workloads.make_config(a.config)
    c0 = np.ascontiguousarray(C[0])
    N = c0.size // 3
    with pkg.Context(0) as ctx:
        ctx.set_points(x, y, w)
        # the identity first: the per-disk values add up to the closure's area, bit for bit
        owned, excl, area = ctx.area_by_disk(c0)
        want = ctx.area(c0)
        assert float(np.sum(owned)) == area == want, (float(np.sum(owned)), area, want)
        assert np.all(excl <= owned)
        for _ in range(a.warmup):
            ctx.area(c0)
            ctx.area_by_disk(c0)
        t_area, t_by = [], []
        for _ in range(a.rounds):   # alternating blocks: drift hits both alike
            t_area.append(block(ctx.area, c0, a.calls))
            t_by.append(block(ctx.area_by_disk, c0, a.calls))
        # kernel spans, profiled apart from the timed blocks
        ctx.profile(True)
        spans = {}
        for name, fn in (("closure_kernel", ctx.area), ("by_disk_kernel", ctx.area_by_disk)):
            ctx.profile_read(reset=True)
            for _ in range(200):
                fn(c0)
            ms, launches, _, _ = ctx.profile_read(reset=True)
            spans[name] = ms / launches * 1e3 if launches else None
        ctx.profile(False)
    med_area, med_by = float(np.median(t_area)), float(np.median(t_by))
    k_cl, k_by = spans["closure_kernel"], spans["by_disk_kernel"]
    line = json.dumps({
        "tool": "by_disk_time", "config": a.config, "N": N, "M": int(x.size),
        "rounds": a.rounds, "calls_per_round": a.calls,
        "area_by_disk_call_us": med_by, "area_by_disk_call_us_min_max": [min(t_by), max(t_by)],
        "area_call_us": med_area, "area_call_us_min_max": [min(t_area), max(t_area)],
        "call_ratio": med_by / med_area,
        "by_disk_kernel_us": k_by, "closure_kernel_us": k_cl,
        "kernel_ratio": (k_by / k_cl) if k_by and k_cl else None,
        "area": area, "owned_nonzero": int(np.count_nonzero(owned)),
        "exclusive_below_owned": int(np.count_nonzero(excl < owned)),
        "identity": "sum(owned) == area == Context.area: bit-identical",
    })
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
