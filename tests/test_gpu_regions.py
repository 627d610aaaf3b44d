"""GPU: high-interest regions (mac_set_regions / mac_regions_ingested / mac_region_stats_f64,
csrc/k_regions.h): the importance override as entries arrive (src/CellFunctions.jl:42-45, :68-72)
and the "Percentage of Area Covered" counts (src/FullSimulation.jl:537-557) on the device list.

Every expected value comes from the numpy restatements below (`ref_check`, `ref_override`,
`ref_percentage`), from the oracle's per-entry flags (orc.np_covered), its rmvCoveredPOI
(orc.ref_remove_covered), its objective and its fire, never from another device path. Counts are
compared exactly; weights exactly wherever every partial sum is exact (weights 25 / 100 or powers
of two), else to rtol 1e-12 against the list-order sum.

The session-wide `ctx` is left without regions by every test that sets them (try / finally); the
tests that change an option use a Context of their own."""
import math

import numpy as np
import pytest

import boundary_cases as bc

pytestmark = pytest.mark.gpu

INVAL, SIZE, NOPOINTS = 1, 2, 3
W_HI = 100.0


# ---- literal numpy restatements ----------------------------------------------------------------

def ref_check(x, y, boxes):
    """src/CellFunctions.jl:42 / src/FullSimulation.jl:542 per box: column b is
    p[1] < x_UB[b] && p[1] > x_LB[b] && p[2] < y_UB[b] && p[2] > y_LB[b] for every point."""
    x_LB, x_UB, y_LB, y_UB = (np.asarray(v, dtype=np.float64) for v in boxes)
    p1, p2 = np.asarray(x)[:, None], np.asarray(y)[:, None]
    with np.errstate(invalid="ignore"):
        return (p1 < x_UB[None, :]) & (p1 > x_LB[None, :]) & (p2 < y_UB[None, :]) & (p2 > y_LB[None, :])


def ref_override(rec, boxes, w_high):
    """:42-45 / :68-72 over records: if any(check) new_point[4] = w_high (column 4, 1-based)."""
    out = np.array(rec, dtype=np.float64, copy=True)
    hit = ref_check(out[:, 0], out[:, 1], boxes).any(axis=1)
    out[hit, 3] = w_high
    return out


def ref_percentage(pushed_xy, remaining_xy, boxes):
    """:537-557: (total, uncovered, 100 - uncovered / total * 100)."""
    total = int(ref_check(pushed_xy[:, 0], pushed_xy[:, 1], boxes).any(axis=1).sum())
    unc = int(ref_check(remaining_xy[:, 0], remaining_xy[:, 1], boxes).any(axis=1).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return total, unc, float(100 - np.float64(unc) / np.float64(total) * 100)


def seq_sum(v):
    """The list-order sequential sum (np.add.accumulate is sequential)."""
    v = np.asarray(v, dtype=np.float64)
    return float(np.add.accumulate(v)[-1]) if v.size else 0.0


def _recs(x, y, w):
    return np.stack([x, y, w, w, np.zeros_like(x)], axis=1)


def _lattice(pkg, seed=11):
    """The 100 x 100 createPOI lattice (10,000 entries), shuffled with 5 % duplicates."""
    rec = pkg.AreaCoverageCalculation.createPOI(5.0, 5.0, 100.0, 100.0)
    rng = pkg.workloads.SplitMix64(seed)
    return pkg.workloads.shuffled_with_duplicates(rec[:, 0], rec[:, 1], rec[:, 3], rng)


def _seeded_boxes(pkg, n, seed):
    """Edges drawn from multiples of 2.5 in [-5, 510]: many lie exactly on lattice coordinates
    (x = 2.5, 7.5, ...), where strict means out. One in eight keeps lb, ub as drawn (lb >= ub
    possible: an empty box)."""
    rng = pkg.workloads.SplitMix64(seed)
    e = rng.integers(-2, 204, 4 * n).astype(np.float64).reshape(4, n) * 2.5
    xl, xu, yl, yu = e
    keep = rng.integers(0, 7, n) == 0
    xs, ys = np.sort(np.stack([xl, xu]), axis=0), np.sort(np.stack([yl, yu]), axis=0)
    xl, xu = np.where(keep, xl, xs[0]), np.where(keep, xu, xs[1])
    yl, yu = np.where(keep, yl, ys[0]), np.where(keep, yu, ys[1])
    return xl, xu, yl, yu


def _expect_stats(x, y, w, boxes, circles=None, orc=None):
    m = ref_check(x, y, boxes)
    anym = m.any(axis=1)
    out = dict(box_count=m.sum(axis=0), box_weight=np.array([seq_sum(w[m[:, b]]) for b in range(m.shape[1])]),
               any_count=int(anym.sum()), any_weight=seq_sum(w[anym]), covered_count=0, covered_weight=0.0)
    if circles is not None and np.size(circles):
        cov = orc.np_covered(circles, x, y) & anym
        out["covered_count"] = int(cov.sum())
        out["covered_weight"] = seq_sum(w[cov])
    return out


def _assert_stats(got, want, exact=True, where=""):
    assert np.array_equal(got["box_count"], want["box_count"]), where
    assert got["any_count"] == want["any_count"], where
    assert got["covered_count"] == want["covered_count"], where
    if exact:
        assert np.array_equal(got["box_weight"], want["box_weight"]), where
        assert got["any_weight"] == want["any_weight"], where
        assert got["covered_weight"] == want["covered_weight"], where
    else:
        np.testing.assert_allclose(got["box_weight"], want["box_weight"], rtol=1e-12, atol=0, err_msg=where)
        np.testing.assert_allclose([got["any_weight"], got["covered_weight"]],
                                   [want["any_weight"], want["covered_weight"]], rtol=1e-12, atol=0)


# ---- 1. stats against numpy ---------------------------------------------------------------------

@pytest.mark.parametrize("tile_points", [1, 4, 4096])
def test_stats_against_numpy(pkg, orc, tile_points):
    """200 seeded boxes (four calls of 50) on the shuffled lattice, per-box and union counts and
    weights (multiples of 25: exact), again after a remove_covered and after an append."""
    x, y, w = _lattice(pkg)
    B = _seeded_boxes(pkg, 200, 2024)
    batches = [tuple(v[q:q + 50] for v in B) for q in range(0, 200, 50)]
    inside = ref_check(x, y, B)
    on_edge = (np.isin(x[:, None], np.concatenate([B[0], B[1]])).any(axis=1))
    assert inside.any() and on_edge.any() and (B[0] >= B[1]).any()

    def check(c, x, y, w, stage):
        for q, boxes in enumerate(batches):
            c.set_regions(*boxes)
            _assert_stats(c.region_stats(), _expect_stats(x, y, w, boxes), where=f"{stage} batch {q}")

    with pkg.Context(0, tile_points=tile_points) as c:
        c.set_points(x, y, w)
        check(c, x, y, w, "set")
        circles = np.array([120.0, 300.0, 410.0, 130.0, 310.0, 90.0, 60.0, 45.0, 80.0])
        c.clear_regions()
        kept = c.remove_covered(circles)
        assert np.array_equal(kept, orc.ref_remove_covered(circles, _recs(x, y, w)))
        x, y, w = x[kept], y[kept], w[kept]
        check(c, x, y, w, "removed")
        rng = pkg.workloads.SplitMix64(5)
        xa = rng.integers(0, 220, 700).astype(np.float64) * 2.5
        ya = rng.integers(0, 220, 700).astype(np.float64) * 2.5
        c.append_points(xa, ya, np.full(700, 25.0))   # (regions on, w_high = NaN: weights stay)
        x, y, w = np.concatenate([x, xa]), np.concatenate([y, ya]), np.concatenate([w, np.full(700, 25.0)])
        gx, gy, gw = c.get_points()
        assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gw, w)
        check(c, x, y, w, "appended")


# ---- 2. degenerate boxes and lists --------------------------------------------------------------

def _degenerate_boxes():
    nan, inf = math.nan, math.inf
    rows = [
        (100.0, 100.0, 0.0, 500.0),      # lb == ub
        (300.0, 100.0, 0.0, 500.0),      # lb > ub
        (0.0, 500.0, 250.0, 200.0),      # lb > ub in y
        (nan, 500.0, 0.0, 500.0),        # a NaN bound, each position
        (0.0, nan, 0.0, 500.0),
        (0.0, 500.0, nan, 500.0),
        (0.0, 500.0, 0.0, nan),
        (-inf, inf, -inf, inf),          # infinite bounds: every finite entry
        (-inf, 250.0, 100.0, inf),
        (inf, inf, 0.0, 500.0),
        (-inf, -inf, 0.0, 500.0),
        (600.0, 700.0, 0.0, 500.0),      # outside the list's bounding box, every side
        (-300.0, -200.0, 0.0, 500.0),
        (0.0, 500.0, 900.0, 1000.0),
        (0.0, 500.0, -1000.0, -900.0),
        (-1e300, 1e300, -1e300, 1e300),  # holding everything
        (0.0, 500.0, 0.0, 500.0),
        (2.5, 497.5, 2.5, 497.5),        # edges on the outermost lattice coordinates
        (100.0, 200.0, 100.0, 200.0),    # identical boxes
        (100.0, 200.0, 100.0, 200.0),
        (150.0, 300.0, 150.0, 300.0),    # overlapping the two above
        (120.0, 130.0, 120.0, 130.0),    # inside them
        (247.5, 252.5, 247.5, 252.5),    # the gap between four lattice points: nothing
        (247.4, 252.6, 247.4, 252.6),    # ... and just around them: four
    ]
    a = np.array(rows).T
    return tuple(a[q].copy() for q in range(4))


def test_degenerate_boxes(ctx, pkg):
    x, y, w = _lattice(pkg)
    try:
        ctx.set_points(x, y, w)
        boxes = _degenerate_boxes()
        ctx.set_regions(*boxes)
        want = _expect_stats(x, y, w, boxes)
        assert want["box_count"][7] == x.size and want["box_count"][22] == 0
        assert want["any_count"] == x.size          # the union counts every entry once
        _assert_stats(ctx.region_stats(), want)
        # 64 boxes: the 24 above, then 40 seeded ones
        more = _seeded_boxes(pkg, 64 - boxes[0].size, 77)
        b64 = tuple(np.concatenate([more[q], boxes[q]]) for q in range(4))
        assert b64[0].size == 64
        ctx.set_regions(*b64)
        _assert_stats(ctx.region_stats(), _expect_stats(x, y, w, b64))
        # 65 boxes: refused, and the 64 stay
        b65 = tuple(np.concatenate([v, v[:1]]) for v in b64)
        with pytest.raises(pkg.MaxCoverError) as e:
            ctx.set_regions(*b65)
        assert e.value.code == INVAL
        _assert_stats(ctx.region_stats(), _expect_stats(x, y, w, b64))
    finally:
        ctx.clear_regions()


def test_degenerate_lists_and_errors(ctx, pkg):
    nan, inf = math.nan, math.inf
    boxes = ([-inf, 0.0, 10.0, 5.0], [inf, 100.0, 20.0, 5.0], [-inf, -10.0, -1.0, 0.0], [inf, 10.0, 1.0, 9.0])
    lists = {
        "non-finite": (np.array([nan, 1.0, inf, -inf, 50.0, 15.0, nan, 15.0, 1e308]),
                       np.array([0.0, nan, 0.0, 0.0, inf, 0.0, nan, -inf, 0.0])),
        "one entry": (np.array([15.0]), np.array([0.5])),
        "one entry outside": (np.array([150.0]), np.array([50.0])),
        "collinear in y": (np.arange(40.0), np.zeros(40)),            # H = 0
        "collinear in x": (np.full(40, 15.0), np.arange(40.0) - 20),  # W = 0
        "one position": (np.full(7, 12.0), np.full(7, 0.25)),
        "empty": (np.zeros(0), np.zeros(0)),
    }
    try:
        for name, (x, y) in lists.items():
            w = 2.0 ** (np.arange(x.size) % 4)
            ctx.set_regions(*boxes, w_high=nan)
            ctx.set_points(x, y, w)
            circles = np.array([15.0, 0.0, 3.0])
            got = ctx.region_stats(circles)
            m = ref_check(x, y, boxes)
            anym = m.any(axis=1)
            assert np.array_equal(got["box_count"], m.sum(axis=0)), name
            assert got["any_count"] == int(anym.sum()), name
            assert np.array_equal(got["box_weight"], [seq_sum(w[m[:, b]]) for b in range(4)]), name
            with np.errstate(invalid="ignore", over="ignore"):
                dx, dy = x - 15.0, y - 0.0
                cov = (np.sqrt(dx * dx + dy * dy) < 3.0) & anym
            assert got["covered_count"] == int(cov.sum()) and got["covered_weight"] == seq_sum(w[cov]), name
            cnt, tot = ctx.regions_ingested()
            assert np.array_equal(cnt, m.sum(axis=0)) and tot == int(anym.sum()), name
        # errors: three_n % 3, too many disks, regions off, no list
        with pytest.raises(pkg.InexactError) as e:
            ctx.region_stats(np.zeros(4))
        assert e.value.code == SIZE
        ctx.clear_regions()
        for call in (ctx.region_stats, ctx.regions_ingested):
            with pytest.raises(pkg.MaxCoverError) as e:
                call()
            assert e.value.code == INVAL
        with pkg.Context(0) as c2:
            c2.set_regions(*boxes)
            with pytest.raises(pkg.MaxCoverError) as e:
                c2.region_stats()
            assert e.value.code == NOPOINTS
            assert c2.regions_ingested()[1] == 0
    finally:
        ctx.clear_regions()


# ---- 3. weights ---------------------------------------------------------------------------------

def test_weight_sums(ctx, pkg, orc):
    x, y, _ = _lattice(pkg)
    rng = pkg.workloads.SplitMix64(31)
    boxes = _seeded_boxes(pkg, 48, 9)
    circles = np.array([100.0, 350.0, 120.0, 330.0, 70.0, 90.0])
    try:
        ctx.set_regions(*boxes)
        w = 2.0 ** rng.integers(0, 3, x.size).astype(np.float64)   # {1, 2, 4, 8}: every sum exact
        ctx.set_points(x, y, w)
        _assert_stats(ctx.region_stats(circles), _expect_stats(x, y, w, boxes, circles, orc))
        w = rng.uniform(x.size) * 50 + 0.001
        ctx.set_points(x, y, w)
        a = ctx.region_stats(circles)
        b = ctx.region_stats(circles)
        _assert_stats(a, _expect_stats(x, y, w, boxes, circles, orc), exact=False)
        assert a["box_weight"].tobytes() == b["box_weight"].tobytes()
        assert (a["any_weight"], a["covered_weight"]) == (b["any_weight"], b["covered_weight"])
    finally:
        ctx.clear_regions()


# ---- 4. covered ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 12, 64])
def test_covered_on_the_lattice(ctx, pkg, orc, N):
    x, y, w = _lattice(pkg)
    rng = pkg.workloads.SplitMix64(100 + N)
    boxes = ([50.0, 200.0, 0.0], [260.0, 420.0, 500.0], [40.0, 180.0, 300.0], [310.0, 290.0, 332.5])
    cx, cy = rng.uniform(N) * 500, rng.uniform(N) * 500
    r = rng.uniform(N) * 60 + 5
    if N == 1:
        cx[0], cy[0], r[0] = 250.0, 250.0, 60.0
    if N >= 12:   # disks that cover nothing, among those that do
        r[1], r[4], r[7] = 0.0, -3.0, math.nan
        cx[9] = math.nan
        cy[10] = math.inf
    circles = np.concatenate([cx, cy, r])
    try:
        ctx.set_points(x, y, w)
        ctx.set_regions(*boxes)
        want = _expect_stats(x, y, w, boxes, circles, orc)
        assert 0 < want["covered_count"] < want["any_count"]
        _assert_stats(ctx.region_stats(circles), want)
        if N == 1:
            for rr in (0.0, -1.0, math.nan):
                got = ctx.region_stats(np.array([250.0, 250.0, rr]))
                assert got["covered_count"] == 0 and got["covered_weight"] == 0.0
                assert got["any_count"] == want["any_count"]
            with pytest.raises(pkg.MaxCoverError) as e:   # N = 2049
                ctx.region_stats(np.ones(3 * 2049))
            assert e.value.code == INVAL
            got = ctx.region_stats(np.concatenate([np.full(2048, 250.0), np.full(2048, 250.0),
                                                   np.full(2048, 40.0)]))
            one = _expect_stats(x, y, w, boxes, np.array([250.0, 250.0, 40.0]), orc)
            _assert_stats(got, one)
    finally:
        ctx.clear_regions()


@pytest.mark.parametrize("weights", bc.WEIGHTS)
def test_covered_at_the_ulp_boundary(ctx, pkg, orc, weights):
    """The `near` case of tests/boundary_cases.py with one box over all of its targeted entries: an
    entry with a = T(r) is covered, one with a = next_up(T(r)) is not."""
    c = bc.make_case("near", weights)
    t = c.cls != bc.BG
    box = ([c.x[t].min() - 1.0], [c.x[t].max() + 1.0], [c.y[t].min() - 1.0], [c.y[t].max() + 1.0])
    inside = ref_check(c.x, c.y, box)[:, 0]
    assert inside[t].all()
    try:
        ctx.set_points(c.x, c.y, c.w)
        ctx.set_regions(*box)
        for ri, k in enumerate(c.rows):
            cov = orc.np_covered(c.C[k], c.x, c.y)
            # this row's own on / off entries, decided by their disk alone where it is exposed
            mine = np.isin(c.disk, c.disk_of[ri][c.exposed[ri]]) if ri < c.disk_of.shape[0] else np.zeros_like(t)
            assert (cov & mine & (c.cls == bc.ON)).any() and (~cov & mine & (c.cls == bc.OFF)).any()
            want = _expect_stats(c.x, c.y, c.w, box, c.C[k], orc)
            _assert_stats(ctx.region_stats(c.C[k]), want, where=f"row {k}")
    finally:
        ctx.clear_regions()


# ---- 5. ingest ----------------------------------------------------------------------------------

BOX_A = ([100.0, 300.0], [200.0, 450.0], [100.0, 50.0], [200.0, 120.0])
BOX_B = ([0.0], [120.0], [0.0], [500.0])


def _ingest_want(x, y, w, boxes, w_high):
    m = ref_check(x, y, boxes)
    return ref_override(_recs(x, y, w), boxes, w_high)[:, 3], m.sum(axis=0), int(m.any(axis=1).sum())


def _assert_ingest(c, x, y, want_w, want_cnt, want_tot, where):
    gx, gy, gw = c.get_points()
    assert np.array_equal(gx, x) and np.array_equal(gy, y), where
    assert np.array_equal(gw, want_w), where
    cnt, tot = c.regions_ingested()
    assert np.array_equal(cnt, want_cnt) and tot == want_tot, where


def test_ingest_every_entry_point(ctx, pkg):
    import torch
    x, y, w = _lattice(pkg)        # (coordinates 5 i - 2.5 and weights 25: exact in fp32 too)
    dev = torch.device("cuda", 0)
    tx, ty, tw = (torch.tensor(v, dtype=torch.float64, device=dev) for v in (x, y, w))
    fx, fy, fw = (t.to(torch.float32) for t in (tx, ty, tw))
    ww, wc, wt = _ingest_want(x, y, w, BOX_A, W_HI)
    assert 0 < wt < x.size and (ww == W_HI).sum() == wt
    setters = {
        "set_points_f64": lambda: ctx.set_points(x, y, w),
        "set_points_f32": lambda: ctx.set_points_f32(x, y, w),
        "set_points_records_f64": lambda: ctx.set_points_records(_recs(x, y, w)),
        "set_points_dev_f64": lambda: ctx.set_points_device(tx, ty, tw),
        "set_points_dev_f32": lambda: ctx.set_points_device_f32(fx, fy, fw),
    }
    h = x.size // 2
    wwB, wcB, wtB = _ingest_want(x[h:], y[h:], w[h:], BOX_B, 7.0)
    appenders = {
        "append_points_f64": lambda: ctx.append_points(x[h:], y[h:], w[h:]),
        "append_points_dev_f64": lambda: ctx.append_points_device(tx[h:], ty[h:], tw[h:]),
    }
    try:
        for name, f in setters.items():
            ctx.set_regions(*BOX_A, w_high=W_HI)
            ctx.set_points(x[:10], y[:10], w[:10])       # counters that the next set must replace
            f()
            _assert_ingest(ctx, x, y, ww, wc, wt, name)
        for name, f in appenders.items():
            ctx.set_regions(*BOX_A, w_high=W_HI)
            ctx.set_points(x[:h], y[:h], w[:h])
            wa, ca, ta = _ingest_want(x[:h], y[:h], w[:h], BOX_A, W_HI)
            _assert_ingest(ctx, x[:h], y[:h], wa, ca, ta, name)
            # the same boxes: the append adds to the counters
            f()
            _assert_ingest(ctx, x, y, ww, wc, wt, name)
            # other boxes in between: counters zeroed, earlier entries keep what they got under A
            ctx.set_points(x[:h], y[:h], w[:h])
            ctx.set_regions(*BOX_B, w_high=7.0)
            assert ctx.regions_ingested()[1] == 0
            f()
            _assert_ingest(ctx, x, y, np.concatenate([wa, wwB]), wcB, wtB, name + " (boxes changed)")
        # w_high = NaN: counted, not overridden
        ctx.set_regions(*BOX_A)
        ctx.set_points(x, y, w)
        _assert_ingest(ctx, x, y, w, wc, wt, "w_high = NaN")
        ctx.append_points(x[h:], y[h:], w[h:])
        m = ref_check(x[h:], y[h:], BOX_A)
        _assert_ingest(ctx, np.concatenate([x, x[h:]]), np.concatenate([y, y[h:]]), np.concatenate([w, w[h:]]),
                       wc + m.sum(axis=0), wt + int(m.any(axis=1).sum()), "w_high = NaN, append")
        # remove_covered leaves the counters alone; set_regions zeroes them and touches no weight
        ctx.set_regions(*BOX_A, w_high=W_HI)
        ctx.set_points(x, y, w)
        kept = ctx.remove_covered(np.array([150.0, 150.0, 60.0]))
        assert kept.size < x.size
        _assert_ingest(ctx, x[kept], y[kept], ww[kept], wc, wt, "after remove_covered")
        ctx.set_regions(*BOX_A, w_high=W_HI)
        _assert_ingest(ctx, x[kept], y[kept], ww[kept], np.zeros(2, dtype=np.int64), 0, "after set_regions")
        # cleared: a new list keeps its weights
        ctx.clear_regions()
        ctx.set_points(x, y, w)
        assert np.array_equal(ctx.get_points()[2], w)
        ctx.append_points(x[h:], y[h:], w[h:])
        assert np.array_equal(ctx.get_points()[2], np.concatenate([w, w[h:]]))
    finally:
        ctx.clear_regions()


def test_ingest_from_the_fire(ctx, pkg, orc):
    """Fire.step(append_to=): the points arrive through the device append and are overridden as the
    reference's update_POI pushes them (:68-72)."""
    fire = pkg.Fire(90, 90, 5.0, 5.0, 0.7, 0.5, 4.0, math.radians(270), (35, 50, 40, 45), 99)
    boxes = ([150.0], [260.0], [150.0], [230.0])
    try:
        ctx.set_regions(*boxes, w_high=W_HI)
        init = fire.initial_points()
        ctx.set_points_records(init)
        lst = [init]
        for _ in range(12):
            fire.step(append_to=ctx)
            lst.append(fire.last_points())
        full = np.concatenate(lst)
        want = ref_override(full, boxes, W_HI)
        hit = want[:, 3] == W_HI
        assert 0 < hit.sum() < full.shape[0] and hit[init.shape[0]:].any()
        gx, gy, gw = ctx.get_points()
        assert np.array_equal(np.stack([gx, gy, gw], axis=1), want[:, [0, 1, 3]])
        cnt, tot = ctx.regions_ingested()
        assert tot == int(hit.sum()) and cnt[0] == tot
        assert ctx.region_stats()["any_weight"] == W_HI * tot
    finally:
        ctx.clear_regions()
        fire.close()


# ---- 6. the objective sees it -------------------------------------------------------------------

def test_objective_sees_the_override(ctx, pkg, orc):
    """w_high = 100 beside weights of 25: every sum exact, so area, poll_best and mads_run on the
    overridden device list equal the oracle on numpy-overridden records bit for bit."""
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    wl = pkg.workloads
    x, y, w = _lattice(pkg)
    boxes = ([180.0, 40.0], [330.0, 110.0], [150.0, 380.0], [290.0, 460.0])
    rec = ref_override(_recs(x, y, w), boxes, W_HI)
    assert 0 < (rec[:, 3] == W_HI).sum() < x.size
    N = 6
    rng = wl.SplitMix64(8)
    x0 = np.round(np.concatenate([rng.uniform(N) * 300 + 100, rng.uniform(N) * 300 + 100,
                                  rng.uniform(N) * 20 + 15]))
    r_max = np.full(N, 30.0 * bc.TAN50)
    cands = wl.poll_candidates(x0, rng)
    try:
        ctx.set_regions(*boxes, w_high=W_HI)
        ctx.set_points(x, y, w)
        assert ctx.area(x0) == orc.ref_area(x0, rec) != orc.ref_area(x0, _recs(x, y, w))
        assert np.array_equal(ctx.area_batch(cands), orc.PointerList(rec).area_batch(cands))
        want = np.array([orc.ref_objective(c, rec, r_max) for c in cands])
        bo, bi, objs = ctx.poll_best(cands, r_max, want_all=True)
        assert np.array_equal(objs, want)
        assert bi == int(np.argmin(want)) and bo == want[bi]
        kw = dict(n_iter=12, ell0=2, ell_max=6, seed=4242)
        x_out, st = ctx.mads_run(x0, r_max, 1e5, prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=bc.TAN50, **kw)
        c3 = TC.create_cons3(x0, 100 / 180 * math.pi, np.full(N, 10.0))
        res = TS.mads(x0, lambda v: orc.ref_objective(v, rec, r_max, 1e5), [c3], N_iter=12, ell0=2,
                      ell_max=6, seed=4242)
        assert np.array_equal(x_out, res.x if res.x is not None else res.i)
        assert st["f"] == res.x_cost
    finally:
        ctx.clear_regions()


# ---- 7. end to end ------------------------------------------------------------------------------

PARENT_RECORD_KEYS = {
    "t", "points", "added", "kept", "f", "iterations", "evaluations", "feasible_evaluations",
    "rejected_polls", "successes", "rounds", "useful_feasible_evaluations",
    "speculative_feasible_evaluations", "slot_fallbacks", "fire_s", "remove_s", "mads_s", "step_s",
    "mads_host_s", "input"}
TIMED = {"fire_s", "remove_s", "mads_s", "step_s", "mads_host_s"}


def _replay(pkg, orc, D, x0, boxes, w_high, steps, N_iter, seed, poll_vars="xyr", granularity=None):
    """The MPC loop on the host: the oracle's fire, the numpy override at every push,
    ref_remove_covered, and the per-trial-point MADS loop on the oracle's objective. poll_vars
    ("auto": FullSimulation.auto_poll_vars per step, as Simulation chooses) and granularity are passed
    through to TDM_STATIC_opt.mads; each row then holds the step's poll_vars."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    N = x0.size // 3
    tan = math.tan(FS.FOV / 2)
    ref = orc.RefFire(D.grid_size[0], D.grid_size[1], ignition=D.ignition, seed=pkg.DynamicArea.SEED)

    def push(rows):
        return ref_override(rows, boxes, w_high) if boxes is not None else rows

    lst = push(D.initial_points())
    pushed = lst[:, :2].copy()
    r_max = np.full(N, FS.h_max * tan)
    d_lim = np.full(N, 10.0)
    x_prev, outputs, out = x0.copy(), [], []
    for t in range(1, steps + 1):
        new = push(ref.step())
        lst = np.concatenate([lst, new])
        pushed = np.concatenate([pushed, new[:, :2]])
        kept = orc.ref_remove_covered(x_prev, lst)
        lst = lst[kept]
        if t != 1:
            FS.r_max_update(x_prev, r_max, N, boxes)
        inp = x_prev
        if t >= 3 and FS.cons3_ok(x_prev, outputs[-1], d_lim):
            inp = outputs[-1]
        rec = lst.copy()
        rm = r_max.copy()
        c3 = TC.create_cons3(x_prev, FS.FOV, d_lim)
        more = {}
        if poll_vars != "xyr":
            g = pkg._lib.mesh_granularity(granularity, x0.size)
            more["poll_vars"] = poll_vars if poll_vars != "auto" else \
                FS.auto_poll_vars(inp[2 * N:], r_max, 1.0 if g is None else g[2 * N:])
        if granularity is not None:
            more["granularity"] = granularity
        res = TS.mads(inp, lambda v: orc.ref_objective(v, rec, rm, 1e5), [c3], N_iter=N_iter, ell0=2,
                      ell_max=6, seed=seed + t, **more)
        x_out = res.x if res.x is not None else res.i
        outputs.append(x_out)
        row = dict(t=t, points=lst.shape[0], added=new.shape[0], kept=kept.size, f=res.x_cost,
                   lst=lst.copy(), x=x_out, input=inp.copy(), **more)
        if boxes is not None:
            row["hi_total"], row["hi_uncovered"], row["hi_percentage"] = ref_percentage(pushed, lst, boxes)
        out.append(row)
        x_prev = x_out
    return out


@pytest.mark.parametrize("high", [True, False])
def test_simulation_end_to_end(ctx, pkg, orc, high):
    """A 64 x 64-cell fire, 6 UAVs, 3 MPC steps of 10 MADS iterations, a box the fire crosses,
    w_high = 100: outputs and hi_* records equal the host replay; without high_interest the records
    have the parent's keys and the replay's values without any override."""
    FS = pkg.FullSimulation
    tan = math.tan(FS.FOV / 2)
    x0 = np.round(orc.ref_allocate_even_circles(40.0, 6, 10 * tan, 160.0, 160.0))
    boxes = ([100.0], [220.0], [60.0], [165.0]) if high else None   # (its upper edge cuts the ignition block)
    D = pkg.DynamicArea.DynamicArea(X=320, Y=320, x_start1=130, x_start2=190, y_start1=150, y_start2=175)
    assert D.grid_size == (64, 64)
    try:
        want = _replay(pkg, orc, D, x0, boxes, W_HI, 3, 10, 77)
        kw = dict(high_interest=boxes, w_high=W_HI) if high else {}
        sim = FS.Simulation(ctx, x0, fire=D, N_iter=10, seed=77, **kw)
        for t in range(3):
            rec = sim.step()
            wt = want[t]
            gx, gy, gw = ctx.get_points()
            assert np.array_equal(np.stack([gx, gy, gw], axis=1), wt["lst"][:, [0, 1, 3]]), t
            assert np.array_equal(rec["input"], wt["input"]), t
            assert np.array_equal(sim.outputs[-1], wt["x"]), t
            for k in ("t", "points", "added", "kept", "f"):
                assert rec[k] == wt[k], (t, k)
            if high:
                assert set(rec) == PARENT_RECORD_KEYS | {"hi_total", "hi_uncovered", "hi_percentage"}
                assert (rec["hi_total"], rec["hi_uncovered"]) == (wt["hi_total"], wt["hi_uncovered"]), t
                assert rec["hi_percentage"] == wt["hi_percentage"], t
                assert sim.percentage_covered() == wt["hi_percentage"], t
            else:
                assert set(rec) == PARENT_RECORD_KEYS
        if high:
            last = want[-1]
            assert last["hi_total"] > last["hi_uncovered"] > 0      # the box was crossed and partly covered
            assert (last["lst"][:, 3] == W_HI).any() and (last["lst"][:, 3] == 25.0).any()
        else:
            with pytest.raises(ValueError):
                sim.percentage_covered()
            with pytest.raises(pkg.MaxCoverError):   # no region call was made: regions are off
                ctx.regions_ingested()
    finally:
        ctx.clear_regions()
        D.close()
