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
    ap.add_argument("--ab", default=None, help="(optional) tools/ab.sh's logs")
    ap.add_argument("--plain5", default=None, help="(optional) A<r>.log / B<r>.log of plain `bench.py --config 5` runs")
    ap.add_argument("--dumps", nargs=2, default=None, metavar=("A_DIR", "B_DIR"),
                    help="(optional) bench.py --dump-outputs directories of the two builds: compared byte for byte")
    ap.add_argument("--plain", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    pl = {v: runs(a.plain, v) for v in "AB"}
    if not a.ab:   # plain runs alone (and config 5's, and the dumped outputs)
        out = {"note": a.note,
               "method": "plain `python bench.py` runs of both builds on one box, alternating, the order swapped "
                         "each round; A = the parent's libmaxcover.so, B = this change's",
               "plain_runs": pl,
               "plain_ms_per_step": verdict([r["ms_per_step"] for r in pl["A"]], [r["ms_per_step"] for r in pl["B"]])}
        keys = ["plain_ms_per_step"]
        if a.plain5:
            p5 = {v: runs(a.plain5, v) for v in "AB"}
            out["config5_runs"] = p5
            out["config5_ms_per_step"] = verdict([r["ms_per_step"] for r in p5["A"]], [r["ms_per_step"] for r in p5["B"]])
            keys.append("config5_ms_per_step")
        for k in keys:   # B inside A's own spread: no cost
            v = out[k]
            v["B_median_inside_A_spread"] = min(v["A"]) <= v["B_median"] <= max(v["A"])
        if a.dumps:
            names = sorted(os.path.relpath(p, a.dumps[0]) for p in glob.glob(os.path.join(a.dumps[0], "**", "*"), recursive=True)
                           if os.path.isfile(p))
            same = []
            for n in names:
                pb = os.path.join(a.dumps[1], n)
                with open(os.path.join(a.dumps[0], n), "rb") as fa:
                    da = fa.read()
                same.append(os.path.isfile(pb) and open(pb, "rb").read() == da)
            out["dumped_outputs"] = {"files": names, "identical": bool(names) and all(same)}
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        for k in keys:
            print(k, {q: out[k][q] for q in ("A_median", "B_median", "A_range", "B_range", "B_median_inside_A_spread")})
        print("dumped_outputs", out.get("dumped_outputs"))
        return
    ab = {v: runs(a.ab, v) for v in "AB"}
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
