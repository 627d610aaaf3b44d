"""GPU: the swarm constraints on the device (mac_cons: cons8 spacing, cons7 altitude zone;
cons_mask_kernel) and the masked poll, against a numpy restatement of src/TDM_Constraints.jl:142-172.
Everything is exact equality. The yardstick below is written with elementwise dx*dx + dy*dy,
np.sqrt and < (numpy does not fuse), independently of the kernel's threshold form."""
import ctypes
import math
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")


# ---------------------------------------------------------------- the yardstick

def yard_mask(C, d_sep=NAN, zone_y=NAN, zone_r=NAN):
    """feasible[k] of the K x 3N matrix C (row k = [x; y; r])."""
    C = np.asarray(C, dtype=np.float64)
    K, n3 = C.shape
    N = n3 // 3
    ok = np.ones(K, dtype=bool)
    off = ~np.eye(N, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            x, y, r = C[k, :N], C[k, N:2 * N], C[k, 2 * N:]
            if d_sep > 0:
                dx = x[:, None] - x[None, :]
                dy = y[:, None] - y[None, :]
                hor = np.sqrt(dx * dx + dy * dy)
                if np.any((hor < d_sep) & off):
                    ok[k] = False
            if not (math.isnan(zone_y) or math.isnan(zone_r)):
                if np.any((y < zone_y) & (r > zone_r)):
                    ok[k] = False
    return ok


def min_separation(C):
    C = np.asarray(C, dtype=np.float64)
    N = C.shape[1] // 3
    out = np.empty(C.shape[0])
    for k in range(C.shape[0]):
        x, y = C[k, :N], C[k, N:2 * N]
        dx = x[:, None] - x[None, :]
        dy = y[:, None] - y[None, :]
        h = np.sqrt(dx * dx + dy * dy)
        h[np.eye(N, dtype=bool)] = np.inf
        out[k] = h.min()
    return out


# ---------------------------------------------------------------- data

D = 15.0


def grid_cands(N, plant, seed, d=D):
    """len(plant) candidates of N UAVs on a jittered square grid of pitch 1.05 d (jitter +-0.02 d:
    no pair closer than d); where plant[k], one UAV is moved to 0.5..0.99 d from a grid neighbour."""
    rng = np.random.default_rng(seed)
    K = len(plant)
    side = max(2, math.ceil(math.sqrt(N)))
    cell = rng.permutation(side * side)[:N]          # UAV index -> grid cell: index order != x order
    gx, gy = (cell // side).astype(np.float64), (cell % side).astype(np.float64)
    C = np.empty((K, 3 * N))
    for k in range(K):
        x = 100.0 + 1.05 * d * gx + rng.uniform(-0.02, 0.02, N) * d
        y = 50.0 + 1.05 * d * gy + rng.uniform(-0.02, 0.02, N) * d
        if plant[k] and N > 1:
            i = int(rng.integers(N))
            near = np.flatnonzero((np.abs(gx - gx[i]) + np.abs(gy - gy[i])) == 1)
            j = int(rng.choice(near)) if near.size else (i + 1) % N
            ang = rng.uniform(0, 2 * math.pi)
            rad = rng.uniform(0.5, 0.99) * d
            x[i], y[i] = x[j] + rad * math.cos(ang), y[j] + rad * math.sin(ang)
        C[k, :N], C[k, N:2 * N], C[k, 2 * N:] = x, y, 36.0
    return C


def dev_mask(ctx, C, cons):
    K, n3 = C.shape
    d_c = torch.tensor(C, dtype=torch.float64, device="cuda")
    d_f = torch.full((max(K, 1),), 9, dtype=torch.uint8, device="cuda")
    ctx.cons_mask_dev(d_c, n3, K, cons, d_f)
    torch.cuda.synchronize()
    return d_f.cpu().numpy()[:K].astype(bool)


def check_mask(ctx, C, both_classes=True, **cons):
    want = yard_mask(C, **cons)
    if both_classes:
        rej = 1.0 - want.mean()
        assert 0.1 <= rej <= 0.9, f"yardstick rejects {rej:.2f}: the case does not hold both classes"
    got = ctx.cons_mask(C, cons)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.array_equal(dev_mask(ctx, C, cons), want)
    return want


# ---------------------------------------------------------------- boundary known answers

def pair(x0, y0, x1, y1):
    return np.array([[x0, x1, y0, y1, 1.0, 1.0]])


def test_pythagorean_boundary(ctx):
    C = pair(0.0, 0.0, 9.0, 12.0)
    assert ctx.cons_mask(C, {"d_sep": 15.0}).tolist() == [True]
    assert ctx.cons_mask(C, {"d_sep": math.nextafter(15.0, INF)}).tolist() == [False]
    assert yard_mask(C, 15.0).tolist() == [True]
    assert yard_mask(C, math.nextafter(15.0, INF)).tolist() == [False]


def test_threshold_conversion_on_random_pairs(ctx):
    rng = np.random.default_rng(5)
    for _ in range(200):
        p = rng.standard_normal(4) * 10.0 ** rng.uniform(-3, 3)
        C = pair(*p)
        dx, dy = p[0] - p[2], p[1] - p[3]
        s = float(np.sqrt(np.float64(dx * dx + dy * dy)))
        assert ctx.cons_mask(C, {"d_sep": s}).tolist() == [True], p
        assert ctx.cons_mask(C, {"d_sep": math.nextafter(s, INF)}).tolist() == [False], p


def test_coincident_single_and_off(ctx):
    C = pair(3.0, 4.0, 3.0, 4.0)
    assert ctx.cons_mask(C, {"d_sep": 15.0}).tolist() == [False]
    assert ctx.cons_mask(C, {"d_sep": 5e-324}).tolist() == [False]
    one = np.array([[3.0, 4.0, 1.0]])                       # N = 1: no pairs
    assert ctx.cons_mask(one, {"d_sep": 15.0}).tolist() == [True]
    assert ctx.cons_mask(one, {"d_sep": INF}).tolist() == [True]
    for off in (0.0, -0.0, -1.0, NAN):
        assert ctx.cons_mask(C, {"d_sep": off}).tolist() == [True]
        assert dev_mask(ctx, C, {"d_sep": off}).tolist() == [True]
    assert ctx.cons_mask(C, None).tolist() == [True]
    assert dev_mask(ctx, C, None).tolist() == [True]


def test_extreme_spacings_match_the_yardstick(ctx):
    C = np.array([
        [0.0, 1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0],          # finite pairs
        [0.0, NAN, INF, 0.0, 5.0, 0.0, 1.0, 1.0, 1.0],          # one finite UAV only
        [0.0, 1e200, -1e200, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0],     # dx*dx overflows
        [0.0, 1e-200, 5.0, 0.0, 0.0, 5.0, 1.0, 1.0, 1.0],       # dx*dx underflows to 0
        [0.0, 3e-200, 5.0, 0.0, 0.0, 5.0, 1.0, 1.0, 1.0],
        [1e308, -1e308, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0],     # x_i - x_j overflows
    ])
    for d in (INF, 1e200, 1.7e308, 1e-200, 2e-200, 5e-324, 1.0, 1.0000000000000002):
        want = yard_mask(C, d)
        assert np.array_equal(ctx.cons_mask(C, {"d_sep": d}), want), d
    assert not yard_mask(C, INF)[0] and yard_mask(C, INF)[1]
    # dx = 1e-200 squares to 0: sqrt(0) < 2e-200 holds although |dx| is not far below d_sep, and at
    # d_sep = 1e-200 although |dx| >= d_sep: the sweep's cut must be off where d_sep*d_sep underflows
    assert not yard_mask(C, 2e-200)[3] and not yard_mask(C, 1e-200)[3]


# ---------------------------------------------------------------- shapes

SHAPES = [(2, 6), (3, 6), (63, 6), (64, 6), (65, 6), (512, 6), (2048, 4),
          (32, 63), (32, 64), (32, 65), (32, 3073), (512, 130)]


@pytest.mark.parametrize("N,K", SHAPES)
def test_shapes_on_a_jittered_grid(ctx, N, K):
    rng = np.random.default_rng(1000 * N + K)
    plant = rng.random(K) < 0.5
    plant[:2] = [False, True]
    check_mask(ctx, grid_cands(N, plant, seed=N + K), d_sep=D)


def test_single_candidate_both_ways(ctx):
    """K = 1 cannot hold both classes in one call: one feasible and one infeasible matrix."""
    a = check_mask(ctx, grid_cands(32, [False], seed=1), both_classes=False, d_sep=D)
    b = check_mask(ctx, grid_cands(32, [True], seed=2), both_classes=False, d_sep=D)
    assert a.tolist() == [True] and b.tolist() == [False]


# ---------------------------------------------------------------- where the only close pair sits

def spread(N, pitch=2.0 * D):
    side = math.ceil(math.sqrt(N))
    i = np.arange(N)
    return 100.0 + pitch * (i // side), 50.0 + pitch * (i % side)


@pytest.mark.parametrize("N", [64, 512])
def test_position_of_the_only_violating_pair(ctx, N):
    x0, y0 = spread(N)
    # far apart in index, adjacent in x: index N-5 sits in the last grid column, 3 in the first
    pairs = [(0, 1), (N - 2, N - 1), (0, N - 1), (3, N - 5)]
    rows = []
    for (i, j) in pairs:
        for dy in (12.0, math.nextafter(12.0, 0.0), 11.0):   # exactly 15 (feasible), a hair closer, closer
            x, y = x0.copy(), y0.copy()
            x[j], y[j] = x[i] + 9.0, y[i] + dy
            rows.append(np.concatenate([x, y, np.full(N, 36.0)]))
    C = np.array(rows)
    want = check_mask(ctx, C, d_sep=D)
    assert want.reshape(len(pairs), 3)[:, 0].all() and not want.reshape(len(pairs), 3)[:, 2].any()


def test_one_column_of_uavs_at_exactly_the_spacing(ctx):
    """512 UAVs share one x (the sweep's cut never fires: every pair is tested), y spaced exactly
    d_sep; then one UAV a ulp closer to its neighbour."""
    N = 512
    x = np.full(N, 777.0)
    y = np.arange(N) * D
    rows = [np.concatenate([x, y, np.full(N, 36.0)])]
    for i in (1, 300, N - 1):
        y2 = y.copy()
        y2[i] = math.nextafter(y2[i], 0.0)
        rows.append(np.concatenate([x, y2, np.full(N, 36.0)]))
    want = check_mask(ctx, np.array(rows), d_sep=D)
    assert want.tolist() == [True, False, False, False]


# ---------------------------------------------------------------- non-finite coordinates

def test_non_finite_and_negative_zero(ctx):
    N = 16
    x0, y0 = spread(N)
    rows = []
    for real_violation in (False, True):
        for kind in ("nan_x", "inf_y", "neg_zero", "nan_on_top", "two_inf"):
            x, y = x0.copy(), y0.copy()
            if real_violation:
                x[12], y[12] = x[2] + 3.0, y[2] + 4.0
            if kind == "nan_x":
                x[5] = NAN
            elif kind == "inf_y":
                y[7] = INF
            elif kind == "neg_zero":
                x[0], y[0] = -0.0, -0.0
                x[1], y[1] = 0.0, 40.0
            elif kind == "nan_on_top":      # would coincide with UAV 9 if its x were a number
                x[5], y[5] = NAN, y[9]
            elif kind == "two_inf":         # inf - inf = NaN between them
                x[5], x[6] = INF, INF
                y[5], y[6] = y[6], y[6]
            rows.append(np.concatenate([x, y, np.full(N, 36.0)]))
    # -0.0 against +0.0 at distance 0: a real violation through signed zeros
    x, y = x0.copy(), y0.copy()
    x[0], y[0], x[1], y[1] = -0.0, -0.0, 0.0, 0.0
    rows.append(np.concatenate([x, y, np.full(N, 36.0)]))
    C = np.array(rows)
    want = check_mask(ctx, C, d_sep=D)
    assert want[:5].all() and not want[5:].any()


# ---------------------------------------------------------------- cons7 and the combination

def test_cons7_strictness_off_and_combination(ctx):
    zy, zr = 200.0, 19 * math.tan(100 / 180 * math.pi / 2)
    up = math.nextafter(zr, INF)
    below = math.nextafter(zy, 0.0)

    def row(ys, rs, xs=(0.0, 100.0, 200.0, 300.0)):
        return np.concatenate([xs, ys, rs])

    C = np.array([
        row([zy, zy, 300.0, 300.0], [up, up, up, up]),             # y == zone_y: outside the zone
        row([below, 10.0, 300.0, 300.0], [zr, zr, up, up]),        # r == zone_r: allowed
        row([300.0, 300.0, 300.0, below], [1.0, 1.0, 1.0, up]),    # the last UAV breaks it
        row([below, 300.0, 300.0, 300.0], [up, 1.0, 1.0, 1.0]),    # the first
        row([NAN, 10.0, 300.0, 300.0], [up, NAN, up, up]),         # NaN never satisfies a comparison
        row([10.0, 300.0, 300.0, 300.0], [INF, 1.0, 1.0, 1.0]),
    ])
    want = check_mask(ctx, C, zone_y=zy, zone_r=zr)
    assert want.tolist() == [True, True, False, False, True, False]
    for off in ({"zone_y": NAN, "zone_r": zr}, {"zone_y": zy, "zone_r": NAN}, {"zone_y": zy}):
        assert ctx.cons_mask(C, off).all()
    # with cons8: none / only 7 / only 8 / both
    C2 = np.array([
        row([300.0, 300.0, 300.0, 300.0], [up, up, up, up]),
        row([10.0, 300.0, 300.0, 300.0], [up, 1.0, 1.0, 1.0]),
        row([300.0, 300.0, 300.0, 300.0], [1.0, 1.0, 1.0, 1.0], xs=(0.0, 5.0, 200.0, 300.0)),
        row([10.0, 10.0, 300.0, 300.0], [up, 1.0, 1.0, 1.0], xs=(0.0, 5.0, 200.0, 300.0)),
    ])
    want = check_mask(ctx, C2, d_sep=D, zone_y=zy, zone_r=zr)
    assert want.tolist() == [True, False, False, False]
    assert yard_mask(C2, d_sep=D).tolist() == [True, True, False, False]
    assert np.array_equal(ctx.cons_mask(C2, {"d_sep": D}), yard_mask(C2, d_sep=D))


# ---------------------------------------------------------------- the masked poll

@pytest.fixture(scope="module", params=[(8, 96), (32, 192)], ids=["N8_K49", "N32_K193"])
def poll_case(request, pkg, ctx):
    N, G = request.param
    wl = pkg.workloads
    rng = wl.SplitMix64(7 + N)
    x, y, w = wl.grid_points(G)
    x0 = wl.clustered_disks(N, G, rng)
    C = wl.poll_candidates(x0, rng)
    assert C.shape == (6 * N + 1, 3 * N)
    r_max = np.full(N, 30.0 * np.tan(100 / 180 * np.pi / 2))
    d_sep = float(np.median(min_separation(C)))
    d_sep = math.nextafter(d_sep, INF)
    ctx.set_points(x, y, w)
    return dict(N=N, C=C, r_max=r_max, d_sep=d_sep, x0=x0, pts=(x, y, w))


def expected(objs, mask, idx_base=0):
    o = np.where(mask, objs, np.inf)
    k = int(np.argmin(o))
    return (float(o[k]), k + idx_base, o) if o[k] < np.inf else (INF, -1, o)


def test_masked_poll_equals_plain_poll_with_inf_substituted(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    mask = yard_mask(c["C"], c["d_sep"])
    assert 0.1 <= 1 - mask.mean() <= 0.9
    _, _, objs = ctx.poll_best(c["C"], c["r_max"], want_all=True)
    wo, wi, wobjs = expected(objs, mask)
    bo, bi, got = ctx.poll_best(c["C"], c["r_max"], want_all=True, cons={"d_sep": c["d_sep"]})
    assert (bo, bi) == (wo, wi) and np.array_equal(got, wobjs)
    assert ctx.poll_best(c["C"], c["r_max"], cons={"d_sep": c["d_sep"]}) == (wo, wi)


def test_masked_poll_with_cons3(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    N = c["N"]
    tan = math.tan(100 / 180 * math.pi / 2)
    kw = dict(prev=c["x0"], d_lim=np.full(N, 4.5), tan_half_fov=tan)
    _, _, objs = ctx.poll_best(c["C"], c["r_max"], want_all=True, **kw)
    assert np.isinf(objs).any() and np.isfinite(objs).any()       # cons3 rejects some, not all
    mask = yard_mask(c["C"], c["d_sep"])
    assert (np.isfinite(objs) & ~mask).any()                       # and cons8 rejects some of the rest
    wo, wi, wobjs = expected(objs, mask)
    bo, bi, got = ctx.poll_best(c["C"], c["r_max"], want_all=True, cons={"d_sep": c["d_sep"]}, **kw)
    assert (bo, bi) == (wo, wi) and np.array_equal(got, wobjs)


def test_masked_lower_duplicate_loses_to_the_higher(ctx, poll_case):
    """Two UAVs parked outside the point grid cover nothing, so moving one of them changes the
    spacing and not the objective: row 0 = the best feasible row with that pair too close."""
    c = poll_case
    ctx.set_points(*c["pts"])
    N = c["N"]
    C = c["C"].copy()
    C[:, 0], C[:, N] = -1000.0, -1000.0
    C[:, 1], C[:, N + 1] = -900.0, -1000.0
    _, b, objs = ctx.poll_best(C, c["r_max"], want_all=True)
    d = float(min_separation(C)[b])                                 # strict <: the plain winner stays feasible
    mask = yard_mask(C, d)
    assert mask[b] and not mask.all()
    low = C[b].copy()
    low[1] = -1000.0 + 0.25 * d                                     # UAV 1 next to UAV 0
    C2 = np.vstack([low[None, :], C, C[b][None, :]])
    mask2 = yard_mask(C2, d)
    assert not mask2[0] and mask2[b + 1] and mask2[-1]
    po, pi, pobjs = ctx.poll_best(C2, c["r_max"], want_all=True)
    assert pobjs[0] == pobjs[b + 1] == pobjs[-1] and (po, pi) == (pobjs[0], 0)   # plain: the lowest
    bo, bi, got = ctx.poll_best(C2, c["r_max"], want_all=True, cons={"d_sep": d})
    assert (bo, bi) == (pobjs[b + 1], b + 1)
    assert np.array_equal(got, np.where(mask2, pobjs, np.inf))


def test_everything_masked(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    bo, bi, objs = ctx.poll_best(c["C"], c["r_max"], want_all=True, cons={"d_sep": INF})
    assert (bo, bi) == (INF, -1) and np.all(objs == INF)


def test_constraints_off_is_the_plain_poll(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    plain = ctx.poll_best(c["C"], c["r_max"], want_all=True)
    for cons in (None, {"d_sep": 0.0}, {"d_sep": NAN, "zone_y": 1.0}, {}):
        got = ctx.poll_best(c["C"], c["r_max"], want_all=True, cons=cons)
        assert got[:2] == plain[:2] and np.array_equal(got[2], plain[2])
    # the C entry point with a NULL descriptor
    K, n3 = c["C"].shape
    dp = ctypes.POINTER(ctypes.c_double)
    objs = np.empty(K)
    bo, bi = ctypes.c_double(), ctypes.c_int64()
    rc = ctx._L.mac_poll_best_cons_f64(ctx._h, c["C"].ctypes.data_as(dp), n3, K,
                                       c["r_max"].ctypes.data_as(dp), 1e5, None, None, 1.0,
                                       objs.ctypes.data_as(dp), ctypes.byref(bo), ctypes.byref(bi), None)
    assert rc == 0 and (bo.value, bi.value) == plain[:2] and np.array_equal(objs, plain[2])


def test_device_form_idx_base_and_fetch(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    K, n3 = c["C"].shape
    mask = yard_mask(c["C"], c["d_sep"])
    _, _, objs = ctx.poll_best(c["C"], c["r_max"], want_all=True)
    d_c = torch.tensor(c["C"], dtype=torch.float64, device="cuda")
    d_r = torch.tensor(c["r_max"], dtype=torch.float64, device="cuda")
    for base, cons in ((0, {"d_sep": c["d_sep"]}), (1000, {"d_sep": c["d_sep"]}), (1000, {"d_sep": INF}),
                       (7, None)):
        m = mask if cons and cons["d_sep"] < INF else (np.zeros(K, bool) if cons else np.ones(K, bool))
        wo, wi, wobjs = expected(objs, m, base)
        d_best = torch.zeros(2, dtype=torch.float64, device="cuda")
        d_obj = torch.zeros(K, dtype=torch.float64, device="cuda")
        ctx.poll_best_dev(d_c, n3, K, d_r, d_best, idx_base=base, d_obj=d_obj, cons=cons)
        fo, fi = ctx.best_fetch(d_best)
        torch.cuda.synchronize()
        hb = d_best.cpu().numpy()
        assert (fo, fi) == (wo, wi)
        assert (float(hb[0]), int(hb.view(np.int64)[1])) == (wo, wi)    # the fetch equals a copy of d_best
        assert np.array_equal(d_obj.cpu().numpy(), wobjs)
        # without d_obj the result is the same
        d_best2 = torch.zeros(2, dtype=torch.float64, device="cuda")
        ctx.poll_best_dev(d_c, n3, K, d_r, d_best2, idx_base=base, cons=cons)
        assert ctx.best_fetch(d_best2) == (wo, wi)
        torch.cuda.synchronize()


def test_four_host_threads_on_one_context(ctx, poll_case):
    c = poll_case
    ctx.set_points(*c["pts"])
    seps = np.quantile(min_separation(c["C"]), [0.2, 0.4, 0.6, 0.8])
    _, _, objs = ctx.poll_best(c["C"], c["r_max"], want_all=True)
    masks = [yard_mask(c["C"], float(d)) for d in seps]
    assert len({m.tobytes() for m in masks}) == 4                   # four different problems
    want = [expected(objs, m) for m in masks]
    got = [None] * 4

    def work(t):
        out = []
        for _ in range(5):
            out.append(ctx.poll_best(c["C"], c["r_max"], want_all=True, cons={"d_sep": float(seps[t])}))
        got[t] = out

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for t in range(4):
        assert got[t] is not None
        for bo, bi, o in got[t]:
            assert (bo, bi) == want[t][:2] and np.array_equal(o, want[t][2])


# ---------------------------------------------------------------- error codes

def test_error_codes(pkg, ctx, poll_case):
    lib = pkg._lib
    ctx.set_points(*poll_case["pts"])
    cons = {"d_sep": D}
    big = np.zeros((1, 3 * 2049))
    with pytest.raises(pkg.MaxCoverError) as ei:
        ctx.cons_mask(big, cons)
    assert ei.value.code == lib.MAC_E_INVAL
    with pytest.raises(pkg.MaxCoverError) as ei:
        ctx.poll_best(big, np.zeros(2049), cons=cons)
    assert ei.value.code == lib.MAC_E_INVAL
    assert ctx.cons_mask(np.zeros((1, 3 * 2048)), cons).tolist() == [False]
    with pytest.raises(pkg.InexactError) as ei:
        ctx.cons_mask(np.zeros((1, 4)), cons)
    assert ei.value.code == lib.MAC_E_SIZE
    # K = 0: nothing written
    out = np.full(4, 7, dtype=np.uint8)
    cs = lib.make_cons(cons)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = ctx._L.mac_cons_mask_f64(ctx._h, np.zeros(6).ctypes.data_as(dp), 6, 0, ctypes.byref(cs),
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    assert rc == 0 and np.all(out == 7)
    d_f = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    ctx.cons_mask_dev(torch.zeros(6, dtype=torch.float64, device="cuda"), 6, 0, cons, d_f)
    torch.cuda.synchronize()
    assert np.all(d_f.cpu().numpy() == 7)


def test_no_point_list(pkg):
    lib = pkg._lib
    C = grid_cands(8, [False, True, False, True], seed=3)
    with pkg.Context(0) as fresh:
        assert np.array_equal(fresh.cons_mask(C, {"d_sep": D}), yard_mask(C, D))   # no list needed
        for cons in ({"d_sep": D}, None):
            with pytest.raises(pkg.MaxCoverError) as ei:
                fresh.poll_best(C, np.full(8, 36.0), cons=cons)
            assert ei.value.code == lib.MAC_E_NOPOINTS
