"""Per-UAV attribution (mac_area_by_disk_*: by_disk_kernel, csrc/k_bydisk.h) against the oracle.

owned[i]: the weight of the entries whose first covering disk in index order is disk i — the
credits the reference's loop sums (src/AreaCoverageCalculation.jl:67-78, `break` at the first hit).
exclusive[i]: the weight of the entries disk i alone covers (area(all) - area(all but i)).

Expected values, two independent ways (oracle/oracle.py, unchanged):
  numpy  cov[i] = np_covered(disk i alone): owned[i] = sum w[cov[i] & ~cov[:i].any(0)],
         exclusive[i] = sum w[cov[i] & (cov.sum(0) == 1)], summed in list order;
  C      owned[i] = ref_area(disks[0..i]) - ref_area(disks[0..i-1]),
         exclusive[i] = ref_area(all) - ref_area(all but i)   (exact for equal weights).
Equal weights: bit-exact (counts times the weight). Weighted: rtol 1e-12, the tolerance DESIGN.md §2
states for weighted areas (the kernel sums in tile order, the oracle in list order).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TAN50 = math.tan(100 / 180 * math.pi / 2)


def seq_sum(v) -> float:
    v = np.asarray(v, dtype=np.float64)
    return float(np.add.accumulate(v)[-1]) if v.size else 0.0


def np_by_disk(orc, c, x, y, w):
    """(owned, exclusive, area) from the numpy oracle's per-disk covered flags."""
    c = np.asarray(c, dtype=np.float64)
    N = c.size // 3
    cov = np.zeros((N, x.size), dtype=bool)
    for i in range(N):
        cov[i] = orc.np_covered(np.array([c[i], c[N + i], c[2 * N + i]]), x, y)
    ncov = cov.sum(0)
    owned, excl = np.zeros(N), np.zeros(N)
    before = np.zeros(x.size, dtype=bool)
    for i in range(N):
        owned[i] = seq_sum(w[cov[i] & ~before])
        excl[i] = seq_sum(w[cov[i] & (ncov == 1)])
        before |= cov[i]
    return owned, excl, seq_sum(w[before])


def sub(c, idx):
    """The candidate holding disks `idx` of candidate c, in that order."""
    c = np.asarray(c, dtype=np.float64)
    N = c.size // 3
    idx = np.asarray(idx, dtype=np.int64)
    return np.concatenate([c[idx], c[N + idx], c[2 * N + idx]])


def c_by_disk(orc, c, x, y, w):
    """(owned, exclusive, area) from the C restatement's areas (exact for equal weights)."""
    N = np.asarray(c).size // 3
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    pre = [0.0] + [orc.ref_area(sub(c, np.arange(i + 1)), rec) for i in range(N)]
    owned = np.array([pre[i + 1] - pre[i] for i in range(N)])
    excl = np.array([pre[N] - (orc.ref_area(sub(c, np.delete(np.arange(N), i)), rec) if N > 1 else 0.0)
                     for i in range(N)])
    return owned, excl, pre[N]


def check_exact(ctx, orc, c, x, y, w, with_c=True):
    """ctx holds (x, y, w), equal weights: bit-exact against both oracles; returns the result."""
    owned, excl, area = ctx.area_by_disk(c)
    wo, wx, wa = np_by_disk(orc, c, x, y, w)
    print("by_disk", np.asarray(c).size // 3, "owned", owned.tolist(), "exclusive", excl.tolist(), area)
    assert np.array_equal(owned, wo), (owned, wo)
    assert np.array_equal(excl, wx), (excl, wx)
    assert area == wa
    if with_c:
        co, cx, ca = c_by_disk(orc, c, x, y, w)
        assert np.array_equal(owned, co), (owned, co)
        assert np.array_equal(excl, cx), (excl, cx)
        assert area == ca
    assert area == ctx.area(c)                     # bit for bit mac_area_f64's
    assert float(np.sum(owned)) == area            # (multiples of the weight: exact in any order)
    assert np.all(excl <= owned)
    return owned, excl, area


@pytest.fixture(autouse=True)
def _auto_algo(ctx):
    ctx.set_algo("auto")
    yield


@pytest.fixture(scope="module")
def case1(pkg, orc):
    """96 x 96 lattice (M = 9,216, w = 25), 13 clustered disks, and its numpy values."""
    wl = pkg.workloads
    x, y, w = wl.grid_points(96)
    c = wl.clustered_disks(13, 96, wl.SplitMix64(11))
    return dict(x=x, y=y, w=w, c=c, want=np_by_disk(orc, c, x, y, w))


@pytest.mark.parametrize("N", [13, 1, 5])
def test_clustered_tail_waves(ctx, orc, case1, N):
    """N = 13 leaves three idle waves in the last workgroup; N = 1 and 5 a prefix of the disks."""
    x, y, w = case1["x"], case1["y"], case1["w"]
    ctx.set_points(x, y, w)
    c = sub(case1["c"], np.arange(N))
    owned, excl, _ = check_exact(ctx, orc, c, x, y, w)
    assert np.all(owned[:1] > 0)
    if N == 13:
        assert np.array_equal(owned, case1["want"][0])
        assert np.any(excl < owned) and np.any(excl > 0)   # overlapping, not degenerate


def overflow_disks(pkg):
    """80 disks, integer centres in [230, 250]^2, R = 36: every disk overlaps the other 79 (both
    neighbour sides of disks 0 and 79 overflow their 64 slots). Disks 0 and 79: R = 60, centres
    at least 10 apart, so each keeps a crescent of its own."""
    rng = pkg.workloads.SplitMix64(4242)
    N = 80
    cx = rng.integers(230, 250, N).astype(np.float64)
    cy = rng.integers(230, 250, N).astype(np.float64)
    cx[0], cy[0] = 232.0, 233.0
    cx[79], cy[79] = 247.0, 246.0
    r = np.full(N, 36.0)
    r[0] = r[79] = 60.0
    return np.concatenate([cx, cy, r])


def test_neighbour_list_overflow_both_sides(ctx, pkg, orc, case1):
    x, y, w = case1["x"], case1["y"], case1["w"]
    c = overflow_disks(pkg)
    assert math.hypot(c[0] - c[79], c[80] - c[80 + 79]) >= 10
    wo, wx, _ = np_by_disk(orc, c, x, y, w)
    # the lower-overflow path (disk 79 has 79 lower neighbours) and the upper-overflow path (disk 0
    # has 79 upper neighbours) each decide a non-zero value
    assert wo[79] > 0 and wx[0] > 0
    ctx.set_points(x, y, w)
    check_exact(ctx, orc, c, x, y, w)


NESTED = np.array([100.0, 400.0, 400.0, 100.0, 400.0, 400.0, 36.0, 350.0, 36.0])


def test_span_of_more_than_64_tile_rows(ctx, pkg, orc):
    """(400, 400, 350) spans 70 rows of the default 10 m tiles (the row-by-row walk); the third
    disk lies inside it: 0 and 0."""
    x, y, w = pkg.workloads.grid_points(160)
    ctx.set_points(x, y, w)
    owned, excl, _ = check_exact(ctx, orc, NESTED, x, y, w)
    assert np.array_equal(owned, 25.0 * np.array([164, 15380, 0]))
    assert np.array_equal(excl, 25.0 * np.array([164, 15216, 0]))


def test_exact_lattice_kats(ctx, pkg, orc):
    """Integer disks on the half-integer lattice: exact integer counts, no floating point."""
    wl = pkg.workloads
    G = 96
    x, y, w = wl.grid_points(G)
    ctx.set_points(x, y, w)
    disks = [(100, 100, 36), (300, 120, 50), (200, 350, 41), (420, 420, 36), (60, 300, 17)]
    for a in range(len(disks)):
        for b in range(a):
            assert math.hypot(disks[a][0] - disks[b][0], disks[a][1] - disks[b][1]) > disks[a][2] + disks[b][2]
    c = np.array([d[0] for d in disks] + [d[1] for d in disks] + [d[2] for d in disks], dtype=np.float64)
    owned, excl, area = ctx.area_by_disk(c)
    want = np.array([25.0 * orc.lattice_count_np(d, G) for d in disks])
    assert np.all(want > 0)
    assert np.array_equal(owned, want) and np.array_equal(excl, want)
    assert area == 25.0 * orc.lattice_count_np(c.astype(np.int64), G) == ctx.area(c)
    # the nested pair: the big disk alone covers what the small one does not
    G = 160
    x, y, w = wl.grid_points(G)
    ctx.set_points(x, y, w)
    c = sub(NESTED, [1, 2])
    owned, excl, area = ctx.area_by_disk(c)
    big, small = orc.lattice_count_np([400, 400, 350], G), orc.lattice_count_np([400, 400, 36], G)
    assert small > 0
    assert excl[0] == 25.0 * (big - small) and owned[0] == 25.0 * big
    assert owned[1] == 0.0 and excl[1] == 0.0
    # ... and first in index order the small disk owns its entries, exclusive nowhere
    owned, excl, _ = ctx.area_by_disk(sub(NESTED, [2, 1]))
    assert owned.tolist() == [25.0 * small, 25.0 * (big - small)]
    assert excl.tolist() == [0.0, 25.0 * (big - small)]


def test_degenerate_disks(ctx, orc, case1):
    """r = 0, r < 0, NaN radius, NaN centre: 0 and 0, and nothing taken from the others; two
    identical disks: the lower index owns, neither is exclusive."""
    x, y, w = case1["x"], case1["y"], case1["w"]
    ctx.set_points(x, y, w)
    nan = float("nan")
    good = [(240.0, 240.0, 36.0), (262.0, 251.0, 36.0), (262.0, 251.0, 36.0), (150.0, 300.0, 30.0)]
    bad = [(245.0, 245.0, 0.0), (245.0, 245.0, -3.0), (245.0, 245.0, nan), (nan, 245.0, 36.0),
           (245.0, nan, 36.0)]

    def cand(disks):
        return np.array([d[0] for d in disks] + [d[1] for d in disks] + [d[2] for d in disks])

    mixed = [good[0], bad[0], good[1], bad[1], bad[2], good[2], bad[3], good[3], bad[4]]
    c = cand(mixed)
    owned, excl, area = ctx.area_by_disk(c)
    wo, wx, wa = np_by_disk(orc, c, x, y, w)
    assert np.array_equal(owned, wo) and np.array_equal(excl, wx) and area == wa == ctx.area(c)
    for k in (1, 3, 4, 6, 8):
        assert owned[k] == 0.0 and excl[k] == 0.0
    assert owned[2] > 0 and owned[5] == 0.0 and excl[2] == 0.0 and excl[5] == 0.0   # the identical pair
    assert owned[0] > excl[0] > 0 and owned[7] == excl[7] > 0
    base = ctx.area_by_disk(cand(good))
    assert np.array_equal(base[0], owned[[0, 2, 5, 7]]) and np.array_equal(base[1], excl[[0, 2, 5, 7]])
    for b in bad:   # at index 0: the other disks' results are unchanged
        o2, x2, a2 = ctx.area_by_disk(cand([b] + good))
        assert o2[0] == 0.0 and x2[0] == 0.0
        assert np.array_equal(o2[1:], base[0]) and np.array_equal(x2[1:], base[1]) and a2 == base[2]


def test_reference_firepoints(ctx, pkg, orc, firepoints):
    """The reference's FirePoints table, every row (6,276 entries, duplicates kept), under the
    reference's starting ring and under the ring moved onto the early fire (y >= 297.5); and the
    step-1 list (rows 1..10), where the starting ring covers nothing."""
    rec = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints])
    assert rec.shape[0] == 6276
    x, y, w = (np.ascontiguousarray(rec[:, k]) for k in (0, 1, 3))
    c0 = pkg.Base_Functions.allocate_even_circles(15.0, 5, 10 * TAN50, 250.0, 250.0)
    c1 = c0.copy()
    c1[5:10] += 70.0
    ctx.set_points(x, y, w)
    seen = 0.0
    for c in (c0, c1):
        owned, excl, area = check_exact(ctx, orc, c, x, y, w)
        assert area == orc.ref_area(c, rec)
        seen += area
    assert seen > 0
    rec10 = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints[:10]])
    x, y, w = (np.ascontiguousarray(rec10[:, k]) for k in (0, 1, 3))
    assert y.min() == 297.5
    ctx.set_points(x, y, w)
    owned, excl, area = check_exact(ctx, orc, c0, x, y, w)
    assert area == 0.0 and not owned.any()
    owned, excl, area = check_exact(ctx, orc, c1, x, y, w)
    assert area > 0 and np.any(owned > 0)


def test_shuffled_list_with_duplicates(ctx, pkg, orc, case1):
    wl = pkg.workloads
    x, y, w = wl.shuffled_with_duplicates(case1["x"], case1["y"], case1["w"], wl.SplitMix64(5), 0.05)
    assert x.size > case1["x"].size
    ctx.set_points(x, y, w)
    owned, _, _ = check_exact(ctx, orc, case1["c"], x, y, w)
    assert np.any(owned != case1["want"][0])          # duplicates count once per entry


def test_weighted_list(ctx, pkg, orc, case1):
    """Arbitrary weights: fp64 sums in a fixed order — rtol 1e-12 against the list-order sums,
    bit-identical from call to call."""
    x, y = case1["x"], case1["y"]
    w = 1.0 + 49.0 * pkg.workloads.SplitMix64(99).uniform(x.size)
    ctx.set_points(x, y, w)
    c = case1["c"]
    owned, excl, area = ctx.area_by_disk(c)
    wo, wx, wa = np_by_disk(orc, c, x, y, w)
    print("weighted rel err", np.max(np.abs(owned - wo) / np.maximum(wo, 1e-300)), abs(area - wa) / wa)
    assert np.all(wo > 0)
    np.testing.assert_allclose(owned, wo, rtol=1e-12, atol=0)
    np.testing.assert_allclose(excl, wx, rtol=1e-12, atol=0)
    np.testing.assert_allclose(area, wa, rtol=1e-12, atol=0)
    np.testing.assert_allclose(float(np.sum(owned)), ctx.area(c), rtol=1e-12, atol=0)
    np.testing.assert_allclose(area, ctx.area(c), rtol=1e-12, atol=0)
    assert np.all(excl <= owned)
    again = ctx.area_by_disk(c)
    assert np.array_equal(again[0], owned) and np.array_equal(again[1], excl) and again[2] == area


def test_batch_and_device_paths(ctx, pkg, case1):
    """K = 7 distinct candidates: every column equals its single-candidate call, through the host
    batch, the device call on a non-default stream, K = 1, and each output alone."""
    wl = pkg.workloads
    x, y, w = case1["x"], case1["y"], case1["w"]
    ctx.set_points(x, y, w)
    C = np.ascontiguousarray(wl.poll_candidates(case1["c"], wl.SplitMix64(3))[:7])
    K, three_n = C.shape
    N = three_n // 3
    single = [ctx.area_by_disk(c) for c in C]
    so = np.stack([s[0] for s in single])
    sx = np.stack([s[1] for s in single])
    sa = np.array([s[2] for s in single])
    assert np.array_equal(so[0], case1["want"][0]) and np.array_equal(sx[0], case1["want"][1])
    assert len({s[0].tobytes() for s in single}) > 1     # the columns differ
    bo, bx, ba = ctx.area_by_disk_batch(C)
    assert bo.shape == (K, N) and np.array_equal(bo, so) and np.array_equal(bx, sx) and np.array_equal(ba, sa)
    assert np.array_equal(ba, ctx.area_batch(C))
    o1, x1, a1 = ctx.area_by_disk_batch(C[3:4])
    assert np.array_equal(o1[0], so[3]) and np.array_equal(x1[0], sx[3]) and a1[0] == sa[3]
    # device pointers, a side stream
    dev = torch.device("cuda", ctx.device)
    side = torch.cuda.Stream(dev)
    tC = torch.from_numpy(C).to(dev)
    torch.cuda.synchronize(dev)

    def dev_call(Kd, want_o, want_x, want_a):
        tO = torch.full((Kd, N), -1.0, dtype=torch.float64, device=dev) if want_o else None
        tX = torch.full((Kd, N), -1.0, dtype=torch.float64, device=dev) if want_x else None
        tA = torch.full((Kd,), -1.0, dtype=torch.float64, device=dev) if want_a else None
        torch.cuda.synchronize(dev)
        ctx.area_by_disk_dev(tC, three_n, Kd, tO, tX, tA, stream=side.cuda_stream)
        side.synchronize()
        return tuple(None if t is None else t.cpu().numpy() for t in (tO, tX, tA))

    do, dx, da = dev_call(K, True, True, True)
    assert np.array_equal(do, so) and np.array_equal(dx, sx) and np.array_equal(da, sa)
    do, dx, da = dev_call(1, True, True, True)
    assert np.array_equal(do[0], so[0]) and np.array_equal(dx[0], sx[0]) and da[0] == sa[0]
    # nullable outputs: each alone
    do, dx, da = dev_call(K, True, False, False)
    assert dx is None and da is None and np.array_equal(do, so)
    do, dx, da = dev_call(K, False, True, False)
    assert np.array_equal(dx, sx)
    do, dx, da = dev_call(K, False, False, True)
    assert np.array_equal(da, sa)
    L, h = ctx._L, ctx._h
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    only = np.full((K, N), -1.0)
    assert L.mac_area_by_disk_batch_f64(h, C.ctypes.data_as(dp), three_n, K, only.ctypes.data_as(dp), None, None) == 0
    assert np.array_equal(only, so)
    only = np.full((K, N), -1.0)
    assert L.mac_area_by_disk_batch_f64(h, C.ctypes.data_as(dp), three_n, K, None, only.ctypes.data_as(dp), None) == 0
    assert np.array_equal(only, sx)
    onlya = np.full(K, -1.0)
    assert L.mac_area_by_disk_batch_f64(h, C.ctypes.data_as(dp), three_n, K, None, None, onlya.ctypes.data_as(dp)) == 0
    assert np.array_equal(onlya, sa)
    # status codes: no output at all, a length that is no multiple of 3, K = 0 writes nothing
    assert L.mac_area_by_disk_batch_f64(h, C.ctypes.data_as(dp), three_n, K, None, None, None) == pkg._lib.MAC_E_INVAL
    assert L.mac_area_by_disk_f64(h, C.ctypes.data_as(dp), three_n - 1, None, None, onlya.ctypes.data_as(dp)) == pkg._lib.MAC_E_SIZE
    onlya[:] = -1.0
    assert L.mac_area_by_disk_batch_f64(h, C.ctypes.data_as(dp), three_n, 0, None, None, onlya.ctypes.data_as(dp)) == 0
    assert np.all(onlya == -1.0)
    big = np.zeros(3 * 2049)
    with pytest.raises(pkg.MaxCoverError, match="2048"):
        ctx.area_by_disk(big)
    # the mirror
    mo, mx, ma = pkg.AreaCoverageCalculation.calculateAreaByDisk(C[0], ctx)
    assert np.array_equal(mo, so[0]) and np.array_equal(mx, sx[0]) and ma == sa[0]
    with pytest.raises(pkg.InexactError):
        pkg.AreaCoverageCalculation.calculateAreaByDisk(C[0][:-1], ctx)


def test_empty_inputs(ctx, case1):
    """three_n = 0 or an empty list: zeros, as mac_area_f64."""
    ctx.set_points(case1["x"], case1["y"], case1["w"])
    owned, excl, area = ctx.area_by_disk(np.zeros(0))
    assert owned.size == 0 and excl.size == 0 and area == 0.0
    ctx.set_points(np.zeros(0), np.zeros(0), np.zeros(0))
    owned, excl, area = ctx.area_by_disk(case1["c"])
    assert not owned.any() and not excl.any() and area == 0.0 and owned.size == 13


def test_config2_scale(ctx, pkg, orc):
    """BASELINE config 2 (M = 1,048,576, N = 32, one candidate) against numpy."""
    x, y, w, cands, _ = pkg.workloads.make_config(2)
    ctx.set_points(x, y, w)
    owned, excl, area = check_exact(ctx, orc, cands[0], x, y, w, with_c=False)
    assert np.all(owned > 0)


def test_stepper_attribution(ctx, pkg, firepoints):
    """Simulation(attribution=True) on config 1's inputs (tests/test_config1.py): each record's
    owned sums to the area of the step's MADS output on the step's list; off by default."""
    FS = pkg.FullSimulation
    N, N_iter, seed = 5, 30, 20250216
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 10 * TAN50, 250.0, 250.0))
    sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed, attribution=True)
    got_area = 0.0
    for _ in range(2):
        rec = sim.step()
        assert rec["owned"].shape == (N,) and rec["exclusive"].shape == (N,)
        area = ctx.area(sim.outputs[-1])            # the list is unchanged since the step's MADS
        assert float(np.sum(rec["owned"])) == area
        assert np.all(rec["exclusive"] <= rec["owned"])
        got_area += area
    assert got_area > 0
    sim0 = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed)
    for k in range(2):
        rec = sim0.step()
        assert "owned" not in rec and "exclusive" not in rec
        assert set(rec) == set(sim.records[k]) - {"owned", "exclusive"}
        assert np.array_equal(sim0.outputs[k], sim.outputs[k])
