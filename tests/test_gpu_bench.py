"""GPU: a plain bench.py run (config 3, three timed polls) end to end: the result line's contract,
nothing of --full in it, and --dump-outputs = what the last timed poll returned, checked against
the streaming scan on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP, POLLS, SEED = 3, 1, 8, 20250216   # (bench.py's default --polls and --seed)


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(pkg, ctx, tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "3",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0
    K = d["config"]["candidates_per_step"]
    assert d["value"] == pytest.approx(K / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # a plain run: nothing that takes runs of its own
    assert d["full"] is False
    for k in ("roofline", "cpu_baseline", "closure", "host_poll_ms", "check_timed_poll_vs_scan"):
        assert d[k] is None, k

    assert sorted(p.name for p in out_dir.iterdir()) == ["best.npy"]
    best = np.load(out_dir / "best.npy")
    assert best.dtype == np.float64 and best.shape == (2,)
    assert best.tolist() == [d["best"]["objective"], d["best"]["index"]]

    # the same seeded inputs, the last timed poll's set, through the streaming scan
    wl = pkg.workloads
    cfg = wl.CONFIGS[3]
    G, N = cfg["G"], cfg["N"]
    rng = wl.SplitMix64(SEED)
    x0 = wl.uniform_disks(N, G, rng)
    polls = [wl.poll_candidates(x0, rng) for _ in range(POLLS)]
    cands = polls[(WARMUP + STEPS - 1) % POLLS]
    assert cands.shape[0] == K
    tan = float(np.tan(100 / 180 * np.pi / 2))
    ctx.set_points(*wl.grid_points(G))
    ctx.set_algo("scan")
    try:
        bo, bi = ctx.poll_best(cands, np.full(N, 30.0 * tan), 1e5, prev=cands[0],
                               d_lim=np.full(N, 10.0), tan_half_fov=tan)[:2]
    finally:
        ctx.set_algo("auto")
    assert best[0] == bo and int(best[1]) == bi
