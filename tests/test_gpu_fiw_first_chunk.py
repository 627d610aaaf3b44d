"""GPU: the first chunk of fiw_kernel's walk (k_fiw.h: the first row batch's first 512 entries are
loaded ahead of the position phases, together with each entry's row within the batch, and staging
takes both from there; later chunks search the row prefix themselves), at the smallest layouts where
the hand-over can go wrong. Every case runs with equal weights (the counts build keeps the row) and
with mixed weights (the weighted build searches again), through the forced fused chain, areas and
objectives against the C oracle, exactly (the weights are quarters, so every sum is exact).

128 x 128 lattice at 5 m (tiles of about 10 m, four entries each), polls of integer offsets:

  * empty: a disk over a hole in the list (its box has tiles and no entry) and a disk off the grid;
  * chunk512 / chunk513: a box of 11 x 11 tiles topped up with extra entries to exactly 512 (one
    full chunk, all of it preloaded) and 513 (a second chunk of one entry, searched);
  * rows: a box of more than 64 tile rows (a second row batch) beside a box of one row;
  * slices: more than 512 positions on one disk (two slices: the second restages the first chunk);
  * neighbours: disks with 1 lower neighbour, with 4 (handed to fin2_kernel: the entry's row decides
    which entries are shared) and with 5 (decided in place)."""
import math

import numpy as np
import pytest

from test_gpu_fiw_index import _grid, _neighbour_layout, _offsets, _snap
from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
G = 128
CASES = ("empty", "chunk512", "chunk513", "rows", "slices", "neighbours")
EXTRA = 40   # entries beside the lattice in the chunk cases (the same count in both: one tile grid)
_REF = {}


def _spread(N, r0):
    return np.concatenate([np.array([100.0, 320.0, 540.0, 100.0, 320.0, 540.0, 210.0, 430.0])[:N],
                           np.array([250.0, 250.0, 250.0, 400.0, 400.0, 400.0, 320.0, 320.0])[:N], np.full(N, r0)])


def _build(case, pkg):
    wl = pkg.workloads
    rng = wl.SplitMix64(8800 + CASES.index(case))
    x, y, w = wl.grid_points(G)
    N, K, D = 8, 72, (1, 1, 1, 1)
    if case == "empty":
        keep = ~((x > 200) & (x < 300) & (y > 200) & (y < 300))
        x, y = x[keep], y[keep]
        x0 = _spread(N, 12.0)
        x0[0], x0[N] = 250.0, 250.0      # over the hole
        x0[1], x0[N + 1] = -200.0, 320.0  # off the grid
        S, gx0, gy0 = _grid(pkg, x, y)
        assert 14.0 + 2 * S < 50.0
    elif case in ("chunk512", "chunk513"):
        want = int(case[5:])
        far = np.arange(EXTRA)
        xe, ye = 5.0 + 0.05 * far, np.full(EXTRA, 637.3)
        S, gx0, gy0 = _grid(pkg, np.concatenate([x, xe]), np.concatenate([y, ye]))
        cx, cy, r0 = _snap(gx0 + 25.5 * S), _snap(gy0 + 25.5 * S), 48.0
        reach = r0 + 2.0   # Dx = Dy = Dr = 1: the box is the tiles of centre -+ reach
        assert 4.6 * S < reach < 5.4 * S

        def in_box(px, py):
            tx, ty = np.floor((px - gx0) / S), np.floor((py - gy0) / S)
            return ((tx >= math.floor((cx - reach - gx0) / S)) & (tx <= math.floor((cx + reach - gx0) / S)) &
                    (ty >= math.floor((cy - reach - gy0) / S)) & (ty <= math.floor((cy + reach - gy0) / S)))
        base = int(in_box(x, y).sum())
        need = want - base
        assert base == 11 * 11 * 4 and 0 < need <= EXTRA, (base, need)
        xe[:need], ye[:need] = cx + 0.1 + 0.05 * far[:need], cy + 0.3   # inside the box (and the disk)
        x, y = np.concatenate([x, xe]), np.concatenate([y, ye])
        assert _grid(pkg, x, y) == (S, gx0, gy0) and int(in_box(x, y).sum()) == want
        x0 = _spread(N, 20.0)
        x0[0], x0[N], x0[2 * N] = cx, cy, r0
        x0[1], x0[N + 1] = 100.0, 560.0   # (disk 1 of the spread would overlap the box)
    elif case == "rows":
        S, gx0, gy0 = _grid(pkg, x, y)
        assert math.floor((y.max() - gy0) / S) + 1 > 64 and 3.0 < 0.45 * S
        D, K = (2, 0, 1, 1), 64
        x0 = _spread(N, 20.0)
        x0[0], x0[N], x0[2 * N] = 101.0, _snap(gy0 + 20.5 * S), 2.0
        x0[1], x0[N + 1], x0[2 * N + 1] = 320.0, 320.0, 400.0
    elif case == "slices":
        D, K = (4, 4, 4, 4), 1280
        x0 = _spread(N, 30.0)
    elif case == "neighbours":
        N = 18
        cx, cy = _neighbour_layout(*_grid(pkg, x, y), 14.0)
        x0 = np.concatenate([cx, cy, np.full(N, 12.0)])
    else:
        raise KeyError(case)
    off = _offsets(rng, K, N, D)
    if case == "slices":   # some disk has more than 512 distinct offsets: two slices of positions
        t = off.reshape(K, 3, N)
        assert max(np.unique(t[:, :, i], axis=0).shape[0] for i in range(N)) > 512
    return x, y, np.ascontiguousarray(x0[None, :] + off), N


def _reference(case, weighted, pkg, orc):
    """The case's list, poll and the oracle's answers: computed once, read-only."""
    key = (case, weighted)
    if key not in _REF:
        x, y, C, N = _build(case, pkg)
        rng = pkg.workloads.SplitMix64(4242)
        w = 0.25 * rng.integers(1, 32, x.size).astype(np.float64) if weighted else np.full(x.size, 25.0)
        rec = recs(x, y, w)
        rmax = np.full(N, 30.0 * TAN50)
        area = orc.PointerList(rec).area_batch(C)
        obj = -area + orc.violation_batch(C, rmax) * 1e5
        r = dict(x=x, y=y, w=w, C=C, rmax=rmax, area=area, obj=obj)
        for a in r.values():
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("case", CASES)
def test_first_chunk(ctx, pkg, orc, case, weighted):
    r = _reference(case, weighted, pkg, orc)
    C = r["C"]
    ctx.set_points(r["x"], r["y"], r["w"])
    ctx.set_chain("fused")
    try:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        got = ctx.area_batch(C)
        bo, bi, objs = ctx.poll_best(C, r["rmax"], 1e5, want_all=True)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        ctx.profile_read(reset=True)
        ctx.profile(False)
        assert kern.get("fiw_kernel", 0) >= 2, kern
        bad = np.flatnonzero(got != r["area"])
        assert bad.size == 0, (case, weighted, bad[:8], got[bad[:8]], r["area"][bad[:8]])
        assert np.array_equal(objs, r["obj"]), (case, weighted, np.flatnonzero(objs != r["obj"])[:8])
        k = int(np.argmin(r["obj"]))
        assert (bi, bo) == (k, r["obj"][k]), (case, weighted, bi, k)
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)
