"""GPU: fiw_kernel's numbering of the direct table (k_fiw.h: each thread numbers a run of consecutive
slots and writes the key word (dx, dy, dr) of every occupied one; the triple is derived once for the
run's first slot and stepped from there, dr carrying into dy and dy into dx).

Polls of hand-made integer offsets, so the displacement bound D = (Dx, Dy, Dr, Dl) — and with it the
table's (2 Dx + 1)(2 Dy + 1)(Dr + Dl + 1) slots plus the dead one — is known, every bound met exactly
by some candidate. 256 threads number the table, ceil((slots + 1) / 256) slots each:

  * slots + 1 = 255, 256 (one slot per thread, the last thread with and without one), 257, 512 (two
    per thread), 513 (three) and 6070 (Dx = Dy = 8, Dr + Dl = 20: 24 per thread, runs that cross
    several dr rows and a dy row);
  * Dl != Dr, and a zero extent on x (255, 257, 513), on y (257, 513, "flat_y") and on r (512).

Per candidate, the area through the forced fused chain against the exact count of lattice points
inside the union of its disks (numpy, the coordinates and radii are exact in fp64) and against the C
oracle, and the poll's objectives and argmin against the oracle's. All comparisons are exact."""
import math

import numpy as np
import pytest

from test_gpu_fiw_index import _offsets
from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
N, G, K = 8, 128, 96
# case: (slots + 1, (Dx, Dy, Dr, Dl), r0)
CASES = {
    "s255": (255, (0, 63, 1, 0), 30.0),
    "s256": (256, (1, 2, 9, 7), 30.0),
    "s257": (257, (0, 0, 128, 127), 130.0),
    "s512": (512, (3, 36, 0, 0), 30.0),
    "s513": (513, (0, 0, 500, 11), 12.0),
    "s6070": (6070, (8, 8, 12, 8), 30.0),
    "flat_y": (26, (2, 0, 3, 1), 30.0),
}
_REF = {}


def _reference(case, pkg, orc):
    """The case's list, poll, lattice counts and the oracle's answers: computed once, read-only."""
    if case in _REF:
        return _REF[case]
    slots1, D, r0 = CASES[case]
    assert (2 * D[0] + 1) * (2 * D[1] + 1) * (D[2] + D[3] + 1) + 1 == slots1
    rng = pkg.workloads.SplitMix64(7300 + list(CASES).index(case))
    x, y, w = pkg.workloads.grid_points(G)
    x0 = np.concatenate([np.array([100.0, 320.0, 540.0, 100.0, 320.0, 540.0, 210.0, 430.0]),
                         np.array([250.0, 250.0, 250.0, 400.0, 400.0, 400.0, 320.0, 320.0]), np.full(N, r0)])
    off = _offsets(rng, K, N, D)
    for q, lo, hi in ((0, -D[0], D[0]), (1, -D[1], D[1]), (2, -D[3], D[2])):   # every bound is met
        assert off[:, q * N:(q + 1) * N].min() == lo and off[:, q * N:(q + 1) * N].max() == hi
    C = np.ascontiguousarray(x0[None, :] + off)
    # lattice points inside the union of a candidate's disks (d^2 and r^2 are exact: quarters below 2^21)
    count = np.zeros(K, dtype=np.int64)
    for k in range(K):
        cx, cy, r = C[k, :N], C[k, N:2 * N], C[k, 2 * N:]
        d2 = (x[:, None] - cx[None, :]) ** 2 + (y[:, None] - cy[None, :]) ** 2
        count[k] = int(((d2 < (r * r)[None, :]) & (r > 0)[None, :]).any(axis=1).sum())
    rec = recs(x, y, w)
    rmax = np.full(N, 30.0 * TAN50)
    area = orc.PointerList(rec).area_batch(C)
    assert np.array_equal(area, count * w[0])
    obj = -area + orc.violation_batch(C, rmax) * 1e5
    r = dict(x=x, y=y, w=w, C=C, rmax=rmax, area=area, obj=obj)
    for a in r.values():
        a.setflags(write=False)
    _REF[case] = r
    return r


@pytest.mark.parametrize("case", list(CASES))
def test_numbering(ctx, pkg, orc, case):
    r = _reference(case, pkg, orc)
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
        assert bad.size == 0, (case, bad[:8], got[bad[:8]], r["area"][bad[:8]])
        assert np.array_equal(objs, r["obj"]), (case, np.flatnonzero(objs != r["obj"])[:8])
        k = int(np.argmin(r["obj"]))
        assert (bi, bo) == (k, r["obj"][k]), (case, bi, k)
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)
