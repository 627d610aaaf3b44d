"""GPU: the index phases of fiw_kernel (k_fiw.h: the key row into LDS, the neighbour prefilter, the
direct table's clear and mark, the position lookup) at the smallest shapes where each can go wrong,
against the C oracle (the first-hit area, src/AreaCoverageCalculation.jl:63-78; the objective,
src/TDM_STATIC_opt.jl:82-100; +inf for a candidate failing cons3, src/TDM_Constraints.jl:54-75).
Every poll goes through the forced fused chain and the forced five-launch chain, as a matrix and,
where the poll is x0 +- delta B, in basis form (the generated source). All comparisons are exact.

Shapes: N = 8-24 disks on a 64^2-128^2 lattice at 5 m (tiles of about 10 m: mac_diag_grid).

  * K = 64, 255, 256, 257, 767, 769 and 3073: the key row's thread (12 keys) and 16-B boundaries;
    3073 = kFwMaxK + 1 is the only K with the odd last key that thread 0 takes alone.
  * the direct table (hand-made integer offsets, so that the displacement bound D is known):
    offsets at exactly +-D; 6,143 slots (37 x 83 x 2 + the dead one: the largest table the code takes
    that integer offsets can make, kFwDirect = 6,144) against 6,147 (7 x 439 x 2 + 1: the smallest
    they can make past it, the hash); 730 and 4,914 slots (LTMADS ell = 2, 3: inside and past the
    slots cleared ahead of D); radii r0 + dr <= 0, = 1, r0 = 0, r0 = NaN / inf; each with cons3.
  * an escaped key (one half-integer offset): one position per candidate.
  * neighbours: boxes sharing one tile column, one tile row, one corner tile; boxes side by side
    and one tile apart; 4 and 5 lower neighbours (hand-off against in place); a box leaving the grid
    and a disk wholly off it.
  * rows: a box of more than kPollRB = 64 tile rows, more than kFwCH = 512 entries, one row."""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
KS = (64, 255, 256, 257, 767, 769, 3073)
CASES = tuple(f"k{k}" for k in KS) + ("at_d", "slots6143", "slots6147", "ell2", "ell3", "radii", "nonfinite",
                                     "escape", "neighbours", "neighbours_ell2", "rows")
_REF = {}


def _grid(pkg, x, y):
    """(S, gx0, gy0) of the tile grid the library lays over the list (default tile_points = 4)."""
    L = pkg.load_library()
    L.mac_diag_grid.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int64, ctypes.c_int32,
                                                        ctypes.POINTER(ctypes.c_double)]
    L.mac_diag_grid.restype = ctypes.c_int32
    out = (ctypes.c_double * 4)()
    assert L.mac_diag_grid(x.min(), x.max(), y.min(), y.max(), x.size, 4, out) == 0
    return out[0], float(x.min()), float(y.min())


def _offsets(rng, K, N, D, corners=True):
    """K x 3N integer offsets (row 0: none) inside the box D = (Dx, Dy, Dr, Dl), every bound met
    exactly by some disk (the rows after the first: each extreme, in every sign combination)."""
    Dx, Dy, Dr, Dl = D
    off = np.zeros((K, 3 * N))
    off[1:, :N] = rng.integers(-Dx, Dx, (K - 1) * N).reshape(K - 1, N)
    off[1:, N:2 * N] = rng.integers(-Dy, Dy, (K - 1) * N).reshape(K - 1, N)
    off[1:, 2 * N:] = rng.integers(-Dl, Dr, (K - 1) * N).reshape(K - 1, N)
    if corners:
        q = 1
        for sx in (-Dx, Dx):
            for sy in (-Dy, Dy):
                for sr in (-Dl, Dr):
                    i = q % N
                    off[q, i], off[q, N + i], off[q, 2 * N + i] = sx, sy, sr
                    q += 1
    return off


def _ltmads_rows(wl, x0, rng, K, ell):
    rows = [x0[None, :]]
    while sum(r.shape[0] for r in rows) < K:
        rows.append(wl.poll_candidates(x0, rng, ell=ell, include_incumbent=False))
    return np.ascontiguousarray(np.concatenate(rows)[:K])


def _snap(v):
    """To a multiple of 2^-10: sums with the polls' integer offsets stay exact."""
    return round(v * 1024.0) / 1024.0


def _neighbour_layout(S, gx0, gy0, reach):
    """18 disks on the 128^2 lattice whose boxes, for polls with Dx = Dy = Dr = 1 (reach = r0 + 2),
    meet as the module text lists. A box's edge along an axis is the tile of centre -+ reach; every
    reach below ends in the middle of a tile, so no rounding decides a case."""
    def mid(g0, t):   # the middle of tile t
        return g0 + (t + 0.5) * S
    x, y = [], []

    def pair(tx, ty, dtx, dty):
        """Disk a: x reach ends mid tile tx (right) / y mid tile ty (top); disk b's left / bottom
        reach starts dtx / dty tiles further (0: the same tile is shared; None: same centre)."""
        ax, ay = _snap(mid(gx0, tx) - reach), _snap(mid(gy0, ty) - reach)
        x.extend([ax, ax if dtx is None else _snap(mid(gx0, tx + dtx) + reach)])
        y.extend([ay, ay if dty is None else _snap(mid(gy0, ty + dty) + reach)])
    pair(8, 8, 0, None)      # one tile column
    pair(8, 24, None, 0)     # one tile row
    pair(8, 40, 0, 0)        # one corner tile
    pair(24, 8, 1, None)     # side by side
    pair(24, 24, 2, None)    # one tile apart
    # six mutually overlapping disks: the fifth has 4 lower neighbours (handed to fin2), the sixth 5
    for a, b in [(0, 0), (6, 0), (0, 6), (6, 6), (3, 3), (9, 3)]:
        x.append(450.0 + a)
        y.append(450.0 + b)
    x.extend([3.0, -200.0])   # a box leaving the grid, a disk wholly off it
    y.extend([320.0, 320.0])
    return np.array(x), np.array(y)


def _build(case, pkg):
    wl = pkg.workloads
    rng = wl.SplitMix64(9100 + CASES.index(case))
    out = dict(basis=None)
    if case.startswith("k"):
        K = int(case[1:])
        G, N, r = (64, 8, 20.0) if K == 3073 else (96, 12, 36.0)
        x0 = wl.uniform_disks(N, G, rng, radius=r)
        C = _ltmads_rows(wl, x0, rng, K, 3 if K in (257, 769) else 2)
    elif case in ("ell2", "ell3", "neighbours_ell2"):
        G, N = (128, 18) if case == "neighbours_ell2" else (96, 12)
        if case == "neighbours_ell2":
            x, y, w = wl.grid_points(G)
            cx, cy = _neighbour_layout(*_grid(pkg, x, y), 14.0)
            x0 = np.concatenate([cx, cy, np.full(N, 12.0)])
        else:
            x0 = wl.uniform_disks(N, G, rng, radius=36.0)
        Lm, rp, cp = wl.ltmads_basis_parts(3 * N, 3 if case == "ell3" else 2, rng)
        B = Lm[rp][:, cp].astype(np.float64)
        C = np.ascontiguousarray(np.concatenate([x0[None, :] + B.T, x0[None, :] - B.T]))
        out["basis"] = (x0, Lm, rp, cp, 1.0)
    elif case in ("at_d", "slots6143", "slots6147"):
        G, N = 128, 8
        D = {"at_d": (3, 2, 4, 1), "slots6143": (18, 41, 1, 0), "slots6147": (3, 219, 0, 1)}[case]
        assert (2 * D[0] + 1) * (2 * D[1] + 1) * (D[2] + D[3] + 1) + 1 == {"at_d": 211, "slots6143": 6143,
                                                                          "slots6147": 6147}[case]
        x0 = np.concatenate([np.array([100.0, 320.0, 540.0, 100.0, 320.0, 540.0, 210.0, 430.0]),
                             np.array([250.0, 250.0, 250.0, 400.0, 400.0, 400.0, 320.0, 320.0]), np.full(N, 30.0)])
        C = x0[None, :] + _offsets(rng, 80, N, D)
    elif case in ("radii", "nonfinite"):
        # r0 = 2: dr = -2 and -3 give r <= 0 (the dead slot), dr = -1 gives r = 1; r0 = 0: only dr > 0
        # lives; nonfinite: candidate 0's radius of one disk NaN, of another +inf (and its offsets
        # NaN / inf with it)
        G, N = 64, 8
        x0 = wl.uniform_disks(N, G, rng, radius=20.0)
        x0[2 * N + 1], x0[2 * N + 2], x0[2 * N + 3] = 2.0, 0.0, 1.0
        C = x0[None, :] + _offsets(rng, 96, N, (2, 2, 3, 3))
        assert (C[:, 2 * N + 1] <= 0).any() and (C[:, 2 * N + 1] == 1.0).any() and (C[:, 2 * N + 2] > 0).any()
        if case == "nonfinite":
            C[:, 2 * N + 4] = np.where(np.arange(96) % 3 == 0, np.nan, C[:, 2 * N + 4])
            C[0, 2 * N + 5] = np.inf
            C[7, 2 * N + 6] = -np.inf
    elif case == "escape":
        G, N = 96, 12
        x0 = wl.uniform_disks(N, G, rng, radius=36.0)
        C = x0[None, :] + _offsets(rng, 72, N, (2, 2, 2, 2))
        C[9, 4] += 0.5
    elif case == "neighbours":
        G, N = 128, 18
        x, y, w = wl.grid_points(G)
        cx, cy = _neighbour_layout(*_grid(pkg, x, y), 14.0)
        x0 = np.concatenate([cx, cy, np.full(N, 12.0)])
        C = x0[None, :] + _offsets(rng, 72, N, (1, 1, 1, 1))
    elif case == "rows":
        # Dy = 0 (no disk moves in y), Dr = Dl = 1: disk 0 (r0 = 2, its centre in the middle of a
        # tile row) has a box of one row, disk 1 (r0 = 400) the whole grid's 65 rows and 16,384
        # entries, disk 2 (r0 = 60) about 700 entries
        G, N = 128, 8
        x, y, w = wl.grid_points(G)
        S, gx0, gy0 = _grid(pkg, x, y)
        assert math.floor((y.max() - gy0) / S) + 1 > 64 and 2.0 + 1.0 < 0.45 * S
        x0 = wl.uniform_disks(N, G, rng, radius=20.0)
        x0[0], x0[N], x0[2 * N] = 101.0, _snap(gy0 + 20.5 * S), 2.0
        x0[1], x0[N + 1], x0[2 * N + 1] = 320.0, 320.0, 400.0
        x0[2 * N + 2] = 60.0
        C = x0[None, :] + _offsets(rng, 64, N, (2, 0, 1, 1))
    else:
        raise KeyError(case)
    out.update(G=G, N=N, C=np.ascontiguousarray(C))
    return out


def _reference(case, pkg, orc):
    """The case's list, poll and the oracle's answers: computed once, shared by both chains,
    read-only."""
    if case in _REF:
        return _REF[case]
    r = _build(case, pkg)
    C, N = r["C"], r["N"]
    x, y, w = pkg.workloads.grid_points(r["G"])
    rec = recs(x, y, w)
    rmax = np.full(N, 30.0 * TAN50)
    if case == "nonfinite":
        obj = np.array([orc.ref_objective(c, rec, rmax) for c in C])
        area = orc.PointerList(rec).area_batch(C)
        feas = None
    else:
        area = orc.PointerList(rec).area_batch(C)
        obj = -area + orc.violation_batch(C, rmax) * 1e5
        d = C.reshape(C.shape[0], 3, N) - C[0].reshape(1, 3, N)
        move = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (d[:, 2] / TAN50) ** 2).max(axis=1)
        dlim = np.full(N, float(np.median(move)))
        feas = orc.cons3_batch(C[0], C, dlim, TAN50)
        assert 0 < int(feas.sum()) < C.shape[0], int(feas.sum())
        r["dlim"] = dlim
    r.update(x=x, y=y, w=w, rmax=rmax, area=area, obj=obj, feas=feas)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _REF[case] = r
    return r


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("case", CASES)
def test_index_phases(ctx, pkg, orc, case, chain):
    r = _reference(case, pkg, orc)
    C, rmax, K = r["C"], r["rmax"], r["C"].shape[0]
    assert K >= 64 and 8 <= r["N"] <= 24
    ctx.set_points(r["x"], r["y"], r["w"])
    ctx.set_chain(chain)
    try:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        got = ctx.area_batch(C)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        ctx.profile_read(reset=True)
        ctx.profile(False)
        assert ("fiw_kernel" in kern) == (chain == "fused"), kern
        bad = np.flatnonzero(~((got == r["area"]) | (np.isnan(got) & np.isnan(r["area"]))))
        assert bad.size == 0, (case, chain, bad[:8], got[bad[:8]], r["area"][bad[:8]])
        polls = [("plain", {}, r["obj"])]
        if r["feas"] is not None:
            polls.append(("cons3", dict(prev=C[0], d_lim=r["dlim"], tan_half_fov=TAN50),
                          np.where(r["feas"], r["obj"], np.inf)))
        for tag, kw, want in polls:
            bo, bi, objs = ctx.poll_best(C, rmax, 1e5, want_all=True, **kw)
            assert _same(objs, want), (case, chain, tag, np.flatnonzero(objs != want)[:8])
            if not np.isnan(want).any():
                k = int(np.argmin(want))
                assert (bi, bo) == (k, want[k]), (case, chain, tag, bi, k)
            if r["basis"] is not None:   # the same poll from the generated source
                x0, Lm, rp, cp, delta = r["basis"]
                bo, bi, objs = ctx.poll_basis(x0, Lm, rp, cp, delta, rmax, 1e5, want_all=True, **kw)
                assert _same(objs, want), (case, chain, tag, "basis", np.flatnonzero(objs != want)[:8])
                k = int(np.argmin(want))
                assert (bi, bo) == (k, want[k]), (case, chain, tag, "basis", bi, k)
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)
