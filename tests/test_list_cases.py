"""CPU: the list-edge cases and maintenance sequences (tests/list_cases.py) checked against the
oracle alone before the device sees them, and the tile grid build_index chooses (choose_grid,
through the host-only mac_diag_grid) swept over the cases' bounding boxes and over extremes.

Conditions, not measurements: the generator's disks are chosen so that the oracle meets them.

Reference: src/AreaCoverageCalculation.jl:63-78 (calculateArea), src/CellFunctions.jl:81-108
(rmvCoveredPOI), src/TDM_Constraints.jl:54-75 (cons3)."""
import ctypes
import math

import numpy as np
import pytest

import list_cases as lc

DBL_MAX = float(np.finfo(np.float64).max)


def _bbox(c):
    return lc.finite_bbox(c.x, c.y)


def test_generator_is_deterministic_and_cached():
    names = ("aspect", "nonfinite", "heavy_tile")
    first = {n: lc.make_case(n) for n in names}
    assert all(lc.make_case(n) is first[n] for n in names)
    assert not first["aspect"].x.flags.writeable and not first["aspect"].C.flags.writeable
    saved = dict(lc._CASE)
    lc._CASE.clear()
    try:
        for n in names:
            h = lc.make_case(n)
            for k in ("x", "y", "w", "C", "r_max", "prev", "d_lim"):
                assert getattr(first[n], k).tobytes() == getattr(h, k).tobytes(), (n, k)
    finally:
        lc._CASE.update(saved)
    saved = dict(lc._SEQ)
    lc._SEQ.clear()
    try:
        a, b = lc._build_sequence("random2"), lc._build_sequence("random2")
        assert [o["op"] for o in a] == [o["op"] for o in b]
        assert all(np.array_equal(p["C"], q["C"]) for p, q in zip(a, b))
    finally:
        lc._SEQ.update(saved)


@pytest.mark.parametrize("name", lc.CASES)
def test_case_property(name):
    """Each case is the list its row of the table says."""
    c = lc.make_case(name)
    x, y, w = c.x, c.y, c.w
    M = x.size
    assert c.C.shape == (lc.K, 3 * lc.N) == (67, 33) and np.array_equal(c.C[0], c.prev)
    assert M <= 5000 or name == "wide_grid_stride"
    xmn, xmx, ymn, ymx = _bbox(c)
    with np.errstate(over="ignore"):
        W, H = np.float64(xmx) - np.float64(xmn), np.float64(ymx) - np.float64(ymn)
    if name != "nonfinite":
        assert np.all(w == 25.0)
    if name in ("one_point", "two_points"):
        assert M == {"one_point": 1, "two_points": 2}[name]
    elif name == "identical":
        assert M == 1500 and W == 0 and H == 0
    elif name in ("line_x", "line_y"):
        assert M == 700 and ((H == 0 and W > 0) if name == "line_x" else (W == 0 and H > 0))
    elif name == "aspect":
        assert M == 2000 and 5e5 < x.std() < 2e6 and 5e-4 < y.std() < 2e-3
    elif name in ("outlier", "outlier_xy"):
        assert M == 1025 and xmx == 1e300 and np.sort(x)[-2] < 160
        assert (ymn == -1e300) == (name == "outlier_xy")
        assert W / 1000 > 160      # the pitch the far entry forces holds the whole lattice
    elif name == "outlier_1e30":
        half = np.float32(W / 1000 / 2)      # the lattice's fp32 offset from its tile's centre: finite,
        with np.errstate(over="ignore"):      # its square not
            assert M == 1025 and xmx == 1e30 and np.isfinite(half) and np.isinf(half * half)
    elif name in ("span_overflow_x", "span_overflow_xy"):
        assert math.isfinite(xmn) and math.isfinite(xmx) and math.isinf(W)
        assert math.isinf(H) == (name == "span_overflow_xy") and math.isfinite(ymn) and math.isfinite(ymx)
    elif name == "subnormal_span":
        assert set(np.unique(x)) == {0.0, 1e-310} and not y.any() and 0 < W < np.finfo(np.float64).tiny
        assert min((x == 0).sum(), (x != 0).sum()) > 100
    elif name == "offset":
        assert M == 1024 and xmn > 2.0 ** 40 and ymx < -2.0 ** 40 + 1.5
        assert np.array_equal((x - 2.0 ** 40) * 64, np.round((x - 2.0 ** 40) * 64))      # exact coordinates
        assert np.all(c.C[:, 2 * lc.N:] > 0) and c.C[:, 2 * lc.N:].max() < 0.5
    elif name == "nonfinite":
        bad = ~(np.isfinite(x) & np.isfinite(y))
        assert M == 1024 and bad.sum() == 40 and bad[0] and bad[-1]
        assert np.all(w[~bad] == 25.0)
        assert np.array_equal(np.sort(np.log2(w[bad])), np.arange(40.0))
        assert np.isnan(x).any() and np.isnan(y).any() and (x == math.inf).any() and (x == -math.inf).any()
        assert (np.isnan(x) & np.isnan(y)).any() and (np.isinf(x) & np.isinf(y)).any()
        r = c.C[:, 2 * lc.N:]
        assert np.isinf(r).sum() == 2 and ((r > 1e100) & np.isfinite(r)).sum() == 2
    elif name == "heavy_tile":
        pts, cnt = np.unique(np.stack([x, y], axis=1), axis=0, return_counts=True)
        assert M == 576 + 3000 and cnt.max() == 3001 and np.sort(cnt)[-2] == 1
    elif name == "neg_zero":
        assert (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        assert (np.signbit(y) & (y == 0)).any() and xmn < 0 < xmx and ymn < 0 < ymx
        assert np.signbit(c.C[0, 0]) and c.C[0, 0] == 0
    elif name == "wide_grid_stride":
        first = lc.BBOX_BLOCKS * lc.BBOX_BLOCK
        assert M == first + 3
        a = lc.finite_bbox(x[:first], y[:first])
        b = lc.finite_bbox(x[first:], y[first:])
        assert b[0] < a[0] and b[1] > a[1] and b[2] < a[2] and b[3] > a[3]


@pytest.mark.parametrize("name", lc.CASES)
def test_case_is_not_vacuous(orc, name):
    c = lc.make_case(name)
    rec = lc.recs(c.x, c.y, c.w)
    M = c.x.size
    area = orc.PointerList(rec).area_batch(c.C)
    n_cov = area / 25.0            # (only non-finite entries do not weigh 25, and they are never covered)
    assert np.array_equal(n_cov, np.round(n_cov))
    assert np.unique(area).size >= 2
    feas = orc.cons3_batch(c.prev, c.C, c.d_lim, lc.TAN50)
    assert lc.K // 4 <= feas.sum() <= 3 * lc.K // 4 and feas[0]
    finite = np.isfinite(c.x) & np.isfinite(c.y)
    kept = orc.ref_remove_covered(c.C[0], rec)
    kept_finite = int(finite[kept].sum())
    if name in lc.ALL_OR_NONE:
        # every entry gets the same decision: a partial cover cannot exist. Candidates of both kinds
        # instead, and the incumbent covers (its removal empties the list).
        assert set(np.unique(n_cov)) == {0.0, float(M)}
        assert (n_cov == 0).sum() >= lc.K // 4 and (n_cov == M).sum() >= lc.K // 4
        assert kept.size == 0
    else:
        part = (n_cov > 0) & (n_cov < M)
        assert part.sum() >= (lc.K + 1) // 2, part.sum()
        assert 0.1 * finite.sum() <= kept_finite <= 0.9 * finite.sum(), (kept_finite, finite.sum())
    cov = orc.np_covered(c.C[0], c.x, c.y)
    assert not cov[~finite].any()
    if c.box is not None:
        inside = lc.ref_check(c.x, c.y, tuple([v] for v in (c.box[0], c.box[1], c.box[2], c.box[3])))[:, 0]
        assert inside.any()
    if name == "heavy_tile":
        N = lc.N
        one = np.flatnonzero((c.x == 62.5) & (c.y == 57.5))
        assert one.size == 3001
        owners = [i for i in range(N)
                  if orc.np_covered(c.C[0][[i, N + i, 2 * N + i]], c.x[one[:1]], c.y[one[:1]])[0]]
        assert owners == [3, 7]
    if name == "wide_grid_stride":
        assert cov[-3] and cov[-2]        # the extreme entries are covered: a short bounding box loses them
    print(f"\n{name}: M={M} covered min/median/max = {n_cov.min():.0f}/{np.median(n_cov):.0f}/"
          f"{n_cov.max():.0f} feasible {int(feas.sum())}/{lc.K} kept {kept.size}")


@pytest.mark.parametrize("name", lc.SEQUENCES)
def test_sequence_on_the_model(orc, name):
    """The sequence replayed on the host model alone: it removes, grows and shrinks."""
    ops = lc.make_sequence(name)
    model = lc.Model(orc)
    sizes, partial, removals = [], 0, 0
    for op in ops:
        before = model.x.size
        kept = lc.apply_to_model(model, op)
        if op["op"] == "remove":
            removals += 1
            partial += 0 < kept.size < before
        sizes.append(model.x.size)
        assert model.x.size <= 5000
        assert op["C"].shape[0] == 2 * op["C"].shape[1] + 1 >= lc.K and op["probe"].size == 15
    sizes = np.array(sizes)
    if name.startswith("random"):
        assert len(ops) == 30
    assert removals >= 1 and partial >= 0.6 * removals, (partial, removals)
    assert (sizes > 0).sum() >= 0.8 * len(ops)
    d = np.diff(np.concatenate([[0], sizes]))
    assert (d > 0).any() and (d < 0).any()
    print(f"\n{name}: {len(ops)} operations, {removals} removals ({partial} partial), sizes {sizes.tolist()}")


def test_sequences_cover_every_item():
    ops = [o for n in ("stale_route", "mpc", "edges") for o in lc.make_sequence(n)]
    hows = {o.get("how") for o in ops}
    assert {"set_points", "set_points_records", "set_points_device", "set_points_f32", "append_points",
            "append_points_device"} <= hows
    assert {o["op"] for o in ops} == {"set", "append", "remove", "regions", "clear_regions", "polls"}
    app = [o for o in ops if o["op"] == "append"]
    assert {0, 1} <= {o["pts"][0].size for o in app}
    rem = [o for o in ops if o["op"] == "remove"]
    assert any(o["circles"].size == 0 for o in rem) and any(np.isinf(o["circles"]).any() for o in rem)
    assert any(o["circles"].size == 15 for o in rem)
    assert any(a["op"] == b["op"] == "remove" and np.array_equal(a["circles"], b["circles"])
               for a, b in zip(ops, ops[1:]))
    edges = lc.make_sequence("edges")
    assert edges[0]["op"] == "append"                       # onto a context that never had a list
    for o in lc.make_sequence("stale_route") + lc.make_sequence("edges"):
        if o.get("how") == "set_points_f32":
            for v in o["pts"]:
                assert np.array_equal(v.astype(np.float32).astype(np.float64), v)


# ---------------------------------------------------------------------------------- the tile grid

def _grid(pkg, xmn, xmx, ymn, ymx, M, ppt):
    L = pkg.load_library()
    L.mac_diag_grid.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int64, ctypes.c_int32,
                                                        ctypes.POINTER(ctypes.c_double)]
    L.mac_diag_grid.restype = ctypes.c_int32
    out = (ctypes.c_double * 4)()
    assert L.mac_diag_grid(xmn, xmx, ymn, ymx, int(M), int(ppt), out) == 0
    return out[0], out[1], int(out[2]), int(out[3])


def _tiles(pkg, c, r, g0, invS, n):
    """predicate.h's own tile_of(c) and tile_span(c, r) (None: no span), through mac_diag_tiles."""
    L = pkg.load_library()
    L.mac_diag_tiles.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.mac_diag_tiles.restype = ctypes.c_int32
    out = (ctypes.c_int32 * 4)()
    assert L.mac_diag_tiles(c, r, g0, invS, n, out) == 0
    return out[0], ((out[2], out[3]) if out[1] else None)


def _check_grid(pkg, box, M, ppt, points=(), where=""):
    xmn, xmx, ymn, ymx = box
    S, invS, nTx, nTy = _grid(pkg, xmn, xmx, ymn, ymx, M, ppt)
    where = (where, box, M, ppt, S, invS, nTx, nTy)
    tiny = float(np.finfo(np.float64).tiny)
    assert math.isfinite(S) and S >= tiny and math.isfinite(invS) and invS >= tiny, where
    assert nTx >= 1 and nTy >= 1 and nTx * nTy <= lc.grid_cap(M), where
    # the extreme entries land in the first and the last tile at the most, and a disk that covers an
    # entry spans its tile
    for g0, lo, hi, n in ((xmn, xmn, xmx, nTx), (ymn, ymn, ymx, nTy)):
        assert _tiles(pkg, lo, 1.0, g0, invS, n)[0] == 0, where
        ps = [lo, hi, lo / 2 + hi / 2] + [p for p in points if lo <= p <= hi]
        for p in ps:
            t = _tiles(pkg, p, 1.0, g0, invS, n)[0]
            assert 0 <= t < n, where
            for c, r in ((p, 1.0), (p, S), (p, 5e-324), (p, 1e300), (p + S / 2, S), (p - S / 4, S / 2),
                         (p - 1.0, 1.5), (p + 30.0, 36.0)):
                with np.errstate(over="ignore", invalid="ignore"):
                    d = np.float64(p) - np.float64(c)
                    covered = math.isfinite(c) and bool(np.sqrt(d * d) < r)
                if covered:
                    span = _tiles(pkg, c, r, g0, invS, n)[1]
                    assert span is not None and span[0] <= t <= span[1], (where, p, c, r, t, span)
    return S, invS, nTx, nTy


@pytest.mark.parametrize("ppt", [1, 4, 4096])
def test_grid_of_the_cases(pkg, ppt):
    for name in lc.CASES:
        c = lc.make_case(name)
        fx = c.x[np.isfinite(c.x)]
        _check_grid(pkg, _bbox(c), c.x.size, ppt, points=fx[:: max(1, fx.size // 16)].tolist(), where=name)


def test_grid_extremes(pkg):
    """Spans 0, subnormal, tiny, 1, huge and overflowing on either axis, M = 1, 1e3, 2^31 - 2, every
    tile_points: finite positive S and invS and a tile count within the documented cap. (On the
    parent commit the rows with an overflowing span give S = DBL_MAX, a subnormal invS and 1e8 tiles
    on that axis, 1e16 tiles with both, and the rows with a subnormal span invS = inf and 1e8 tiles.)"""
    spans = (0.0, 1e-310, 1e-300, 1.0, 1e300, math.inf)

    def ends(s, origin):
        return (-1.5e308, 1.5e308) if math.isinf(s) else (origin, origin + s)

    for W in spans:
        for H in spans:
            for origin in (0.0, -3.0):
                for M in (1, 1000, 2 ** 31 - 2):
                    for ppt in (1, 4, 4096):
                        _check_grid(pkg, ends(W, origin) + ends(H, origin), M, ppt)
    # the largest finite box, and boxes off to one side of the origin
    _check_grid(pkg, (-DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX), 1000, 4)
    _check_grid(pkg, (1e308, DBL_MAX, -DBL_MAX, -1e308), 1000, 4)
    _check_grid(pkg, (2.0 ** 40, 2.0 ** 40 + 1, -2.0 ** 40, -2.0 ** 40 + 1), 1024, 1)
    # no finite entry, an empty list
    assert _grid(pkg, math.inf, -math.inf, math.inf, -math.inf, 5, 4) == (1.0, 1.0, 1, 1)
    assert _grid(pkg, 0.0, 1.0, 0.0, 1.0, 0, 4) == (1.0, 1.0, 1, 1)


def test_grid_of_ordinary_lists_is_the_parents(pkg):
    """Lists whose grid was right keep it bit for bit: the G x G lattices of bench.py's configurations
    2-4 (G = 1024, 2048, 4096), of smoke() (G = 96) and configuration 5's ignition block, with the values
    of the commit before the fix."""
    parent = {96: (float.fromhex("0x1.3caaaaaaaaaabp+3"), 49), 1024: (9.990234375, 513),
              2048: (9.9951171875, 1025), 4096: (9.99755859375, 2049)}
    for G, (S, n) in parent.items():
        box = (2.5, 5.0 * G - 2.5, 2.5, 5.0 * G - 2.5)
        got = _check_grid(pkg, box, G * G, 4)
        assert got == (S, 1.0 / S, n, n), (G, got)
    # configuration 5's first list: the 512 x 512 ignition block of the 4096 x 4096 grid, cells
    # 1793 .. 2304 on both axes (workloads.config5_setup), entries at 5 i - 2.5
    wl = pkg.workloads
    fire, _ = wl.config5_setup(wl.SplitMix64(wl.SEED))
    lo, hi = fire["x_start1"] - 2.5, fire["x_start2"] - 2.5
    assert (lo, hi) == (8962.5, 11517.5) == (fire["y_start1"] - 2.5, fire["y_start2"] - 2.5)
    got = _check_grid(pkg, (lo, hi, lo, hi), 512 * 512, 4)
    assert got == (9.98046875, 1.0 / 9.98046875, 257, 257), got
