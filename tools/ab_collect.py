"""Collect a same-box A/B (tools/ab.sh's logs, and plain `python bench.py` runs of both builds)
into one JSON file with the acceptance test of a perf change:

    python tools/ab_collect.py --ab bench_out/ab --plain bench_out/plain --out profiles/NAME.json

--ab: A<r>.log / B<r>.log as tools/ab.sh writes them (bench.py --full --no-cpu --no-extras
--steps 40); --plain: A<r>.log / B<r>.log of plain `python bench.py` runs (200 timed polls), A and
B alternating. A is the parent's build, B the change's. B counts as faster on a metric when every
B run is below every A run and the difference of the medians is at least three times the larger
of the two builds' own ranges over those runs.
"""
import argparse
import glob
import json
import os
import statistics


def runs(d, v):
    out = []
    for p in sorted(glob.glob(os.path.join(d, f"{v}[0-9]*.log"))):
        with open(p) as f:
            line = [ln for ln in f if ln.startswith("{")][0]
        j = json.loads(line)
        r = j.get("roofline") or {}
        out.append({"log": os.path.basename(p), "ms_per_step": j["ms_per_step"],
                    "chain_ms": r.get("chain_ms"), "split_ms_per_poll": r.get("split_ms_per_poll"),
                    "kernels_avg_us": {k: v.get("avg_us") for k, v in (r.get("kernels") or j.get("kernels") or {}).items()
                                       if isinstance(v, dict)}})
    return out


def verdict(a, b):
    ra, rb = max(a) - min(a), max(b) - min(b)
    diff = statistics.median(a) - statistics.median(b)
    noise = max(ra, rb)
    return {"A": a, "B": b, "A_median": statistics.median(a), "B_median": statistics.median(b),
            "A_range": ra, "B_range": rb, "median_difference": diff,
            "every_B_below_every_A": max(b) < min(a),
            "difference_over_noise": diff / noise if noise > 0 else None,
            "faster": max(b) < min(a) and diff >= 3.0 * noise}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", required=True)
    ap.add_argument("--plain", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    ab = {v: runs(a.ab, v) for v in "AB"}
    pl = {v: runs(a.plain, v) for v in "AB"}
    out = {"note": a.note,
           "method": "tools/ab.sh A.so B.so 4 (alternating runs on one box, bench.py --full --no-cpu "
                     "--no-extras --steps 40), then plain `python bench.py` three times per build, "
                     "alternating; A = the parent's libmaxcover.so, B = this change's",
           "ab_runs": ab, "plain_runs": pl,
           "chain_us": verdict([r["chain_ms"] * 1e3 for r in ab["A"]], [r["chain_ms"] * 1e3 for r in ab["B"]]),
           "walk_us": verdict([r["split_ms_per_poll"]["walk"] * 1e3 for r in ab["A"]],
                              [r["split_ms_per_poll"]["walk"] * 1e3 for r in ab["B"]]),
           "plain_ms_per_step": verdict([r["ms_per_step"] for r in pl["A"]], [r["ms_per_step"] for r in pl["B"]])}
    keys = ["chain_us", "walk_us", "plain_ms_per_step"]
    # per launch role, where both builds stamped it (the fused chain: prep, fiw, fin2)
    for role in ("prep_kernel", "fiw_kernel", "fin2_kernel"):
        if all(r["kernels_avg_us"].get(role) is not None for v in "AB" for r in ab[v]) and ab["A"] and ab["B"]:
            out[role + "_us"] = verdict([r["kernels_avg_us"][role] for r in ab["A"]],
                                        [r["kernels_avg_us"][role] for r in ab["B"]])
            keys.append(role + "_us")
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for k in keys:
        print(k, {q: out[k][q] for q in ("A_median", "B_median", "A_range", "B_range", "median_difference",
                                         "every_B_below_every_A", "difference_over_noise", "faster")})


if __name__ == "__main__":
    main()
