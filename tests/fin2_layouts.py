"""Layouts for tests/test_gpu_fin2_shared.py (fin2_kernel's shared-entry pass, k_fiw.h), shared with
tools/diag_fiw.py --case NAME, which runs them on the diagnostic build and reports how many disks
were listed (handed off to fin2_kernel) and how many decided their shared entries in place."""
import math

import numpy as np

TAN50 = math.tan(100 / 180 * math.pi / 2)
R = 36.0
CASES = ("pairs", "four_neighbours", "chunks", "weighted", "dead_nonfinite", "batches",
         "batches_weighted")


def _pairs(npairs, G, gap=10.0, pitch=5.0):
    """npairs pairs of disks `gap` apart (integer centres), the pairs on a coarse mesh far from each
    other: disk 2p + 1 has the one lower neighbour 2p."""
    L = pitch * G
    side = int(math.ceil(math.sqrt(npairs)))
    step = L / side
    assert step >= 4 * R + 2 * gap + 40, (G, npairs)
    cx, cy = [], []
    for p in range(npairs):
        ox = round(step * (p % side + 0.5)) + 1.0
        oy = round(step * (p // side + 0.5)) + 2.0
        cx += [ox, ox + gap]
        cy += [oy, oy]
    return np.array(cx), np.array(cy)


def geometry(case, wl):
    """(G, (x, y, w), C, r_max, d_lim) of a case: the lattice side, the point list, the candidate
    matrix (K = 6N + 1; the two-batch cases: its first 97 rows) and cons3's distance limit."""
    ell = 2
    if case in ("pairs", "weighted", "dead_nonfinite"):
        G = 240
        cx, cy = _pairs(6, G)
    elif case == "four_neighbours":
        # two clusters of 5 mutually overlapping disks (the highest of each: 4 lower neighbours)
        # and 3 disks on their own
        G = 240
        off = [(0, 0), (6, 0), (0, 6), (6, 6), (3, 3)]
        cx = [300.0 + a for a, b in off] + [900.0 + a for a, b in off] + [300.0, 900.0, 600.0]
        cy = [300.0 + b for a, b in off] + [900.0 + b for a, b in off] + [900.0, 300.0, 600.0]
        cx, cy = np.array(cx), np.array(cy)
    elif case == "chunks":
        G = 400
        cx, cy = _pairs(12, G)
    elif case in ("batches", "batches_weighted"):
        G = 260
        cx, cy = _pairs(35, G)
    else:
        raise ValueError(case)
    N = cx.size
    x, y, w = wl.grid_points(G)
    seed = 9100 + CASES.index(case)
    rng = wl.SplitMix64(seed)
    if case in ("weighted", "batches_weighted"):
        w = np.array([25.0, 50.0, 75.0])[np.minimum((rng.uniform(w.size) * 3).astype(np.int64), 2)]
    if case == "dead_nonfinite":
        ell = 3
    x0 = np.concatenate([cx, cy, np.full(N, R)])
    C = wl.poll_candidates(x0, rng, ell=ell)
    assert C.shape[0] == 6 * N + 1
    if case in ("batches", "batches_weighted"):   # (the first 97 candidates: the oracle's time)
        C = np.ascontiguousarray(C[:97])
    if case == "dead_nonfinite":   # on listed disks (the higher disk of a pair)
        C[7, 2 * N + 3] = np.nan
        C[20, 2 * N + 5] = -3.0
    # cons3's limit: 10 m (src/FullSimulation.jl:740); at N = 12 an ell = 3 poll fails only 11 of 73
    # candidates under it, so the dead-candidate case takes 9 m, under which 35 of 73 fail
    d_lim = 9.0 if case == "dead_nonfinite" else 10.0
    return G, (x, y, w), C, np.full(N, 30.0 * TAN50), np.full(N, d_lim)
