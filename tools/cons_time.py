"""The swarm-constraint mask (mac_cons_mask_dev_f64, cons_mask_kernel) and the masked poll
(mac_poll_best_cons_dev_f64) against their yardstick, the plain device poll (mac_poll_best_dev_f64),
at config 4 (N = 512, K = 3073, 16.8M entries). Stream-ordered *_dev calls only, timed with device
events over blocks of calls, the three in alternating blocks after a warm-up of all of them.

d_sep is chosen from the data (the per-candidate smallest separation of a 64-candidate sample, numpy):
  "none"  the sample's smallest separation: the numpy yardstick rejects nothing (strict <), so no
          workgroup stops early — the mask's worst case;
  "half"  the sample's median smallest separation (one ulp up): 30-70 % rejected.
Asserts the device mask equals the numpy yardstick on the sample and prints one JSON line.
    python tools/cons_time.py [--config 4] [--rounds 7] [--calls 200] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402


def min_separation(C):
    """Smallest sqrt(dx*dx + dy*dy) over the pairs of each row [x; y; r] (numpy: no fusing)."""
    N = C.shape[1] // 3
    out = np.empty(C.shape[0])
    eye = np.eye(N, dtype=bool)
    for k in range(C.shape[0]):
        x, y = C[k, :N], C[k, N:2 * N]
        dx = x[:, None] - x[None, :]
        dy = y[:, None] - y[None, :]
        h = np.sqrt(dx * dx + dy * dy)
        h[eye] = np.inf
        out[k] = h.min()
    return out


def block_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    x, y, w, C, r_max = pkg.workloads.make_config(a.config)
    K, n3 = C.shape
    N = n3 // 3
    sample = np.linspace(0, K - 1, a.sample).astype(np.int64)
    ms = min_separation(C[sample])
    d_none = float(ms.min())
    d_half = math.nextafter(float(np.median(ms)), math.inf)
    want = {"none": ~(ms < d_none), "half": ~(ms < d_half)}
    assert want["none"].all()
    rej_half = 1.0 - want["half"].mean()
    assert 0.3 <= rej_half <= 0.7, rej_half
    with pkg.Context(0) as ctx:
        ctx.set_points(x, y, w)
        d_c = torch.tensor(C, dtype=torch.float64, device="cuda")
        d_r = torch.tensor(r_max, dtype=torch.float64, device="cuda")
        d_best = torch.zeros(2, dtype=torch.float64, device="cuda")
        d_best2 = torch.zeros(2, dtype=torch.float64, device="cuda")
        d_obj = torch.zeros(K, dtype=torch.float64, device="cuda")
        d_f = torch.zeros(K, dtype=torch.uint8, device="cuda")
        settings = {"none": {"d_sep": d_none}, "half": {"d_sep": d_half}}
        feasible_all = {}
        for name, cons in settings.items():   # the mask against the yardstick first
            ctx.cons_mask_dev(d_c, n3, K, cons, d_f)
            torch.cuda.synchronize()
            got = d_f.cpu().numpy().astype(bool)
            assert np.array_equal(got[sample], want[name]), name
            feasible_all[name] = float(got.mean())
        fns = {"poll_plain": lambda: ctx.poll_best_dev(d_c, n3, K, d_r, d_best, d_obj=d_obj)}
        for name, cons in settings.items():
            cs = pkg._lib.make_cons(cons)
            fns["mask_" + name] = lambda cs=cs: ctx.cons_mask_dev(d_c, n3, K, cs, d_f)
            fns["poll_cons_" + name] = lambda cs=cs: ctx.poll_best_dev(d_c, n3, K, d_r, d_best2,
                                                                        d_obj=d_obj, cons=cs)
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.rounds):   # alternating blocks: drift hits all alike
            for k, fn in fns.items():
                t[k].append(block_us(fn, a.calls))
        # the results the timed calls left behind: the masked poll against the plain one
        ctx.poll_best_dev(d_c, n3, K, d_r, d_best, d_obj=d_obj)
        torch.cuda.synchronize()
        plain = d_obj.cpu().numpy().copy()
        ctx.poll_best_dev(d_c, n3, K, d_r, d_best2, d_obj=d_obj, cons=settings["half"])
        bo, bi = ctx.best_fetch(d_best2)
        torch.cuda.synchronize()
        ctx.cons_mask_dev(d_c, n3, K, settings["half"], d_f)
        torch.cuda.synchronize()
        m = d_f.cpu().numpy().astype(bool)
        o = np.where(m, plain, np.inf)
        assert np.array_equal(d_obj.cpu().numpy(), o) and (bo, bi) == (float(o.min()), int(np.argmin(o)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    line = json.dumps({
        "tool": "cons_time", "config": a.config, "N": N, "K": K, "M": int(x.size),
        "rounds": a.rounds, "calls_per_round": a.calls, "sample": a.sample,
        "d_sep_none": d_none, "d_sep_half": d_half, "sample_rejected_half": rej_half,
        "feasible_fraction_all_K": feasible_all,
        "us_per_call_median": med,
        "us_per_call_min_max": {k: [min(v), max(v)] for k, v in t.items()},
        "mask_none_over_poll_plain": med["mask_none"] / med["poll_plain"],
        "poll_cons_none_over_poll_plain": med["poll_cons_none"] / med["poll_plain"],
        "checks": "mask == numpy yardstick on the sample; masked poll == plain objectives with +inf at "
                  "masked candidates and their numpy argmin",
    })
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
