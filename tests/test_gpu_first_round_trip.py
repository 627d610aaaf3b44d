"""GPU: the first round trip of fiw_kernel (k_fiw.h: the key row and failure words with thread 0's odd
last key, the displacement partials, the lower disks' bases) and of prep_x_kernel (k_prep.h
prep_block_x: prev, rmax and the cons3 threshold ahead of the matrix), at the smallest shapes where
each load's address or predicate can go wrong. Every poll goes through the forced fused chain and the
forced five-launch chain as a matrix and, where it is x0 +- delta B, in basis form. Everything is
compared exactly with the C oracle: the first-hit area (src/AreaCoverageCalculation.jl:63-78), the
objective -area + 1e5 * violation_batch (src/TDM_STATIC_opt.jl:82-100), +inf for a candidate the
oracle's cons3 fails (src/TDM_Constraints.jl:54-75).

  * the odd last key: K = 3072 and 3073 = kFwMaxK + 1 with candidate K - 1 failing and passing cons3
    and with no prev at all (no failure bytes: the clamped byte load reads the key row); K = 64 and
    769 likewise (the extra word and byte are loaded, and dropped, at K <= kFwMaxK).
  * the partials: hand-made integer offsets whose bound D = (24, 2, 2, 1) is met by ONE candidate,
    sitting in the prep workgroup that writes record 0, 255, 256 or the last; K = 6 npd + r for npd =
    1, 255, 256, 257, 511, 512 and r = 0, 5 (and 1 at 512: K = 3073, the largest fused poll; at r = 5
    there, K = 3077, the forced fused chain stands down). A missed record shrinks D from 24 m to 2 m in x, two tiles
    of the box, and the area of that candidate comes out short. A too-large D changes no result, so the
    five-launch side also checks the walk and every disk's position count (mac_diag_poll_report) and
    the fused side that fiw_kernel and fin2_kernel ran (the launches' stamps).
  * the lower disks: N = 258 and 512 at K = 64, all disks far apart but one group: disk N - 1 over
    disk j = 0, 255, 256, N - 2 (one lower neighbour: handed to fin2) or over j and four more (five:
    decided in place).
  * prep's penalty arguments: prev and rmax present / absent, the host API (thresholds made on the
    host, dlimT) against the device API (the raw d_lim), N = 1, 63, 64, 65, 511, 512, K mod 6 = 0, 1, 5;
    d_lim entries of 0, a negative, +inf and NaN; a candidate at exactly d_lim (a 3-4-5 move, d_lim =
    5 and the double below it); a whole-poll rejection through the native driver. The host API takes
    no null r_max (MAC_E_INVAL, asserted), so rmax is absent through the device API only.

Shapes: 64^2 and 128^2 lattices at 5 m; references are computed once per case and shared read-only."""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
_REF = {}


def _freeze(r):
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _profiled(ctx, chain, fn, algo=None):
    """fn() under the forced chain with profiling on: (its result, launches per kernel, hint report)."""
    ctx.set_chain(chain)
    if algo:
        ctx.set_algo(algo)
    try:
        ctx.profile(True)
        ctx.profile_read(reset=True)
        ctx.profile_fused(reset=True)
        out = fn()
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        fused = ctx.profile_fused(reset=True)
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        ctx.set_chain("auto")
        if algo:
            ctx.set_algo("auto")
    return out, kern, fused


def _took(chain, kern, fused, tag):
    """The forced chain ran: fiw_kernel and fin2_kernel on the fused side, the disk index on the
    five-launch side. (The fused chain's hint words reach the host only through a later enqueue under
    AUTO, mac_profile_fused, and may then be an earlier poll's: they are printed, not asserted.)"""
    assert ("fiw_kernel" in kern) == (chain == "fused"), (tag, kern)
    if chain == "fused":
        print(tag, kern, fused)
        assert kern.get("fin2_kernel", 0) == kern["fiw_kernel"], (tag, kern)
    else:
        assert kern.get("disk_index_kernel", 0) > 0, (tag, kern)


def _check_poll(got, want, tag):
    bo, bi, objs = got
    assert _same(objs, want), (tag, np.flatnonzero(objs != want)[:8], objs[:4], want[:4])
    if np.isfinite(want).any():
        k = int(np.argmin(want))
        assert (bi, bo) == (k, want[k]), (tag, bi, bo, k, want[k])
    else:
        assert bi == -1, (tag, bi)


def _inside(rng, K, N, D):
    """K x 3N integer offsets (row 0: none) strictly inside D = (Dx, Dy, Dr, Dl)."""
    Dx, Dy, Dr, Dl = D
    off = np.zeros((K, 3 * N))
    if K > 1:
        n = (K - 1) * N
        off[1:, :N] = np.clip(rng.integers(-(Dx - 1), Dx - 1, n), -(Dx - 1), Dx - 1).reshape(K - 1, N)
        off[1:, N:2 * N] = np.clip(rng.integers(-(Dy - 1), Dy - 1, n), -(Dy - 1), Dy - 1).reshape(K - 1, N)
        off[1:, 2 * N:] = np.clip(rng.integers(-(Dl - 1), Dr - 1, n), -(Dl - 1), Dr - 1).reshape(K - 1, N)
    return off


def _move(C, prev, tan):
    N = prev.size // 3
    d = C.reshape(C.shape[0], 3, N) - prev.reshape(1, 3, N)
    return np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (d[:, 2] / tan) ** 2)


# ------------------------------------------------------------------ 1. the odd last key

LAST_KS = (64, 769, 3072, 3073)
LAST_MODES = ("plain", "last_fails", "last_passes")


def _last_key_ref(pkg, orc, K, mode):
    key = ("last", K, mode)
    if key in _REF:
        return _REF[key]
    wl = pkg.workloads
    rng = wl.SplitMix64(7300 + K)
    G, N, r = (64, 8, 20.0) if K >= 3072 else (96, 12, 36.0)
    x0 = wl.uniform_disks(N, G, rng, radius=r)
    rows = [x0[None, :]]
    while sum(v.shape[0] for v in rows) < K:
        rows.append(wl.poll_candidates(x0, rng, ell=2, include_incumbent=False))
    C = np.ascontiguousarray(np.concatenate(rows)[:K])
    dlim = None
    if mode != "plain":
        dlim = np.full(N, float(np.median(_move(C, x0, TAN50).max(axis=1))))
        # candidate K - 1: every disk 3 m past the limit in x, or one disk a metre off (well inside)
        C[K - 1] = x0
        if mode == "last_fails":
            C[K - 1, :N] += np.ceil(dlim[0]) + 3.0
        else:
            C[K - 1, 0] += 1.0
    x, y, w = wl.grid_points(G)
    rec = recs(x, y, w)
    rmax = np.full(N, 30.0 * TAN50)
    area = orc.PointerList(rec).area_batch(C)
    obj = -area + orc.violation_batch(C, rmax) * 1e5
    kw = {}
    if dlim is not None:
        feas = orc.cons3_batch(x0, C, dlim, TAN50)
        assert bool(feas[K - 1]) == (mode == "last_passes") and 0 < int(feas.sum()) < K
        obj = np.where(feas, obj, np.inf)
        kw = dict(prev=x0, d_lim=dlim, tan_half_fov=TAN50)
    _REF[key] = _freeze(dict(C=C, x=x, y=y, w=w, rmax=rmax, area=area, obj=obj, kw=kw))
    return _REF[key]


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("mode", LAST_MODES)
@pytest.mark.parametrize("K", LAST_KS)
def test_odd_last_key(ctx, pkg, orc, K, mode, chain):
    r = _last_key_ref(pkg, orc, K, mode)
    ctx.set_points(r["x"], r["y"], r["w"])
    tag = (K, mode, chain)
    if mode == "plain":   # (areas alone as well: no objective, no failure bytes)
        got, kern, fused = _profiled(ctx, chain, lambda: ctx.area_batch(r["C"]))
        _took(chain, kern, fused, tag)
        assert _same(got, r["area"]), (tag, np.flatnonzero(got != r["area"])[:8])
    got, kern, fused = _profiled(ctx, chain, lambda: ctx.poll_best(r["C"], r["rmax"], 1e5, want_all=True, **r["kw"]))
    _took(chain, kern, fused, tag)
    _check_poll(got, r["obj"], tag)
    # the last candidate's disks are left out (its objective +inf) or counted (its own area)
    assert np.isinf(got[2][K - 1]) == (mode == "last_fails"), (tag, got[2][K - 1])


# ------------------------------------------------------------------ 2. the partials

D_PART = (24, 2, 2, 1)
NPDS = (1, 255, 256, 257, 511, 512)
PART_CASES = tuple((npd, r, rec) for npd in NPDS for r in ((0, 1, 5) if npd == 512 else (0, 5))
                   for rec in sorted({q for q in (0, 255, 256, npd - 1) if q < npd}))


def _partials_ref(pkg, orc, npd, r, record):
    key = ("part", npd, r, record)
    if key in _REF:
        return _REF[key]
    wl = pkg.workloads
    rng = wl.SplitMix64(8100 + 7 * npd + r)
    G, N, K = 64, 8, 6 * npd + r
    # the centres 60 m apart and 40 m inside the list: the far candidate's disks stay on it
    x0 = np.concatenate([np.array([60.0, 120.0, 180.0, 240.0, 60.0, 120.0, 180.0, 240.0]),
                         np.array([100.0, 100.0, 100.0, 100.0, 220.0, 220.0, 220.0, 220.0]), np.full(N, 20.0)])
    off = _inside(rng, K, N, D_PART)
    # the one candidate at the bound: the first one of workgroup `record` of a matrix prep (six
    # candidates a workgroup; candidate 0 is the base, so record 0 takes candidate 1)
    ks = max(6 * record, 1)
    assert ks < K
    off[ks] = 0.0
    off[ks, 0], off[ks, N], off[ks, 2 * N] = D_PART[0], -D_PART[1], D_PART[2]
    off[ks, 1], off[ks, N + 1], off[ks, 2 * N + 1] = -D_PART[0], D_PART[1], -D_PART[3]
    d = np.abs(off.reshape(K, 3, N))
    assert (d[:, 0].max(axis=1) == D_PART[0]).sum() == 1 and d[np.arange(K) != ks, 0].max() < D_PART[0]
    C = np.ascontiguousarray(x0[None, :] + off)
    x, y, w = wl.grid_points(G)
    rec = recs(x, y, w)
    rmax = np.full(N, 30.0 * TAN50)
    area = orc.PointerList(rec).area_batch(C)
    # the far candidate covers entries a box of the other candidates' reach does not hold
    assert area[ks] != area[0]
    obj = -area + orc.violation_batch(C, rmax) * 1e5
    ucount = np.array([len({C[k, [i, N + i, 2 * N + i]].tobytes() for k in range(K)}) for i in range(N)])
    _REF[key] = _freeze(dict(C=C, x=x, y=y, w=w, rmax=rmax, area=area, obj=obj, ucount=ucount, N=N))
    return _REF[key]


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("npd,r,record", PART_CASES)
def test_partials(ctx, pkg, orc, npd, r, record, chain):
    ref = _partials_ref(pkg, orc, npd, r, record)
    ctx.set_points(ref["x"], ref["y"], ref["w"])
    tag = (npd, r, record, chain)

    def run():
        a = ctx.area_batch(ref["C"])
        rep = ctx.poll_report(ref["N"]) if chain == "five" else None
        return a, rep, ctx.poll_best(ref["C"], ref["rmax"], 1e5, want_all=True)
    (area, rep, got), kern, fused = _profiled(ctx, chain, run, algo="poll")   # (the poll walk at K < 64 too)
    # (K = 6 * 512 + 5 is past kFwMaxK + 1 = 3073 candidates: no fused route, the forced chain stands down)
    _took(chain if ref["C"].shape[0] <= 3073 else "five", kern, fused, tag)
    assert _same(area, ref["area"]), (tag, np.flatnonzero(area != ref["area"])[:8])
    _check_poll(got, ref["obj"], tag)
    if rep is not None:
        assert rep["walk"] == "poll", (tag, rep["walk"])
        assert np.array_equal(rep["ucount"], ref["ucount"]), (tag, rep["ucount"], ref["ucount"])


# ------------------------------------------------------------------ 3. the lower disks

LOWER_CASES = tuple((N, j, nn) for N in (258, 512) for j in ("0", "255", "256", "below") for nn in (1, 5))


def _lower_ref(pkg, orc, N, jname, nn):
    key = ("lower", N, jname, nn)
    if key in _REF:
        return _REF[key]
    wl = pkg.workloads
    rng = wl.SplitMix64(8800 + N)
    G, K = 128, 64
    i = N - 1
    j = i - 1 if jname == "below" else int(jname)
    # sites 20 m apart, radius 2 and moves of at most 1: every box ends 4 m from its centre, 12 m (more
    # than a tile) short of the next one's; the group sits 90 m off the sites
    site = np.arange(N)
    cx, cy = 12.5 + 20.0 * (site % 23), 12.5 + 20.0 * (site // 23)
    rad = np.full(N, 2.0)
    assert cx.max() < 470 and cy.max() < 470
    group = [j] + [q for q in (i - 1, i - 2, i - 3, i - 4, i - 5) if q != j][:nn - 1] + [i]
    assert len(set(group)) == nn + 1 and max(group) == i
    for q, (a, b) in zip(sorted(group), [(0, 0), (6, 0), (0, 6), (6, 6), (3, 3), (9, 3)]):
        cx[q], cy[q], rad[q] = 560.0 + a, 560.0 + b, 12.0
    x0 = np.concatenate([cx, cy, rad])
    C = np.ascontiguousarray(x0[None, :] + _inside(rng, K, N, (2, 2, 2, 2)))
    x, y, w = wl.grid_points(G)
    rec = recs(x, y, w)
    rmax = np.full(N, 30.0 * TAN50)
    area = orc.PointerList(rec).area_batch(C)
    obj = -area + orc.violation_batch(C, rmax) * 1e5
    _REF[key] = _freeze(dict(C=C, x=x, y=y, w=w, rmax=rmax, area=area, obj=obj))
    return _REF[key]


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("N,j,nn", LOWER_CASES)
def test_lower_disks(ctx, pkg, orc, N, j, nn, chain):
    ref = _lower_ref(pkg, orc, N, j, nn)
    ctx.set_points(ref["x"], ref["y"], ref["w"])
    tag = (N, j, nn, chain)
    (area, got), kern, fused = _profiled(
        ctx, chain, lambda: (ctx.area_batch(ref["C"]), ctx.poll_best(ref["C"], ref["rmax"], 1e5, want_all=True)))
    _took(chain, kern, fused, tag)
    assert _same(area, ref["area"]), (tag, np.flatnonzero(area != ref["area"])[:8])
    _check_poll(got, ref["obj"], tag)


# ------------------------------------------------------------------ 4. prep's penalty arguments

PEN_NS = (1, 63, 64, 65, 511, 512)
PEN_KS = (66, 67, 71)   # K mod 6 = 0, 1, 5


def _penalty_ref(pkg, orc, N, K):
    key = ("pen", N, K)
    if key in _REF:
        return _REF[key]
    wl = pkg.workloads
    rng = wl.SplitMix64(9500 + 8 * N + K)
    G = 64
    x0 = wl.uniform_disks(N, G, rng, radius=6.0)
    C = np.ascontiguousarray(x0[None, :] + _inside(rng, K, N, (6, 6, 3, 3)))
    prev = x0.copy()
    prev[:N] += 1.0   # (not candidate 0: every move is measured from elsewhere)
    # UAV 0 stays within 3 m of prev, but for candidate 1: a 3-4-5 move, at exactly d_lim = 5 (passes)
    n = K
    C[:, 0] = prev[0] + rng.integers(-2, 2, n)
    C[:, N] = prev[N] + rng.integers(-2, 2, n)
    C[:, 2 * N] = prev[2 * N] + rng.integers(-1, 1, n)
    C[1, 0], C[1, N], C[1, 2 * N] = prev[0] + 3.0, prev[N] - 4.0, prev[2 * N]
    mv = _move(C, prev, TAN50)   # K x N
    assert mv[1, 0] == 5.0 and mv[np.arange(K) != 1, 0].max() < 4.0
    # every other UAV's limit is its farthest move (all pass), but three that fail their far third
    dlim = mv.max(axis=0)
    for q in {min(2, N - 1), N // 2, N - 1} - {0}:
        dlim[q] = max(np.quantile(mv[:, q], 0.7), mv[1, q])   # (candidate 1 passes them)
    dlim[0] = 5.0
    dlow = dlim.copy()
    dlow[0] = np.nextafter(5.0, 0.0)   # ... and the double below it (fails)
    # d_lim entries of 0 (a UAV that half the candidates leave at prev), +inf and NaN on some UAVs;
    # then a negative one as well (no move passes it)
    dspec, Cs = dlim.copy(), C
    spec = [q for q in (1, N // 3, N - 2) if 0 < q < N]
    if spec:
        Cs = C.copy()
        Cs[::2, [spec[0], N + spec[0], 2 * N + spec[0]]] = prev[[spec[0], N + spec[0], 2 * N + spec[0]]]
        for q, val in zip(spec, (0.0, np.inf, np.nan)):
            dspec[q] = val
    dneg = dspec.copy()
    dneg[N - 1] = -1.0
    x, y, w = wl.grid_points(G)
    rec = recs(x, y, w)
    rmax = np.full(N, 4.0 * TAN50) + np.arange(N) % 3
    pl = orc.PointerList(rec)
    r = dict(C=C, Cs=Cs, x=x, y=y, w=w, rmax=rmax, prev=prev, N=N)
    # (name: candidates, d_lim, the oracle's area, violation and cons3)
    r["polls"] = {name: (cc, dl, pl.area_batch(cc), orc.violation_batch(cc, rmax),
                         orc.cons3_batch(prev, cc, dl, TAN50) if dl is not None else None)
                  for name, cc, dl in (("none", C, None), ("dlim", C, dlim), ("below", C, dlow),
                                       ("special", Cs, dspec), ("negative", Cs, dneg))}
    f, fl, fs, fn = (r["polls"][q][4] for q in ("dlim", "below", "special", "negative"))
    assert f[1] and not fl[1] and np.array_equal(np.delete(f, 1), np.delete(fl, 1))
    assert 0 < f.sum() and (f.sum() < K or N == 1) and not fn.any()
    assert fs.any()   # (d_lim = 0: the candidates that leave that UAV at prev)
    for v in r["polls"].values():
        for a in v:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    _REF[key] = _freeze(r)
    return _REF[key]


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("api", ["host", "device"])
@pytest.mark.parametrize("K", PEN_KS)
@pytest.mark.parametrize("N", PEN_NS)
def test_penalty_arguments(ctx, pkg, orc, N, K, api, chain):
    import torch
    r = _penalty_ref(pkg, orc, N, K)
    ctx.set_points(r["x"], r["y"], r["w"])
    dev = torch.device("cuda", ctx.device)
    if api == "device":
        tCs = {id(c): torch.from_numpy(c.copy()).to(dev) for c in (r["C"], r["Cs"])}
        tR = torch.from_numpy(r["rmax"].copy()).to(dev)
        tP = torch.from_numpy(r["prev"].copy()).to(dev)
        tB = torch.empty(2, dtype=torch.float64, device=dev)
        tO = torch.empty(K, dtype=torch.float64, device=dev)

    def one(C, has_rmax, dl):
        if api == "host":
            kw = dict(prev=r["prev"], d_lim=dl, tan_half_fov=TAN50) if dl is not None else {}
            return ctx.poll_best(C, r["rmax"], 1e5, want_all=True, **kw)
        tD = torch.from_numpy(dl.copy()).to(dev) if dl is not None else None
        ctx.poll_best_dev(tCs[id(C)], 3 * N, K, tR if has_rmax else None, tB, d_prev=tP if dl is not None else None,
                          d_dlim=tD, tan_half_fov=TAN50, d_obj=tO)
        bo, bi = ctx.best_fetch(tB)
        return bo, bi, tO.cpu().numpy()

    for has_rmax in (True, False):
        for name, (C, dl, area, viol, feas) in r["polls"].items():
            tag = (N, K, api, chain, name, has_rmax)
            if api == "host" and not has_rmax:
                # the host API takes no null r_max: the case does not exist there
                L = pkg.load_library()
                bo, bi = ctypes.c_double(), ctypes.c_int64()
                rc = L.mac_poll_best_f64(ctx._h, C.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 3 * N, K, None,
                                         ctypes.c_double(1e5), None, None, ctypes.c_double(TAN50), None,
                                         ctypes.byref(bo), ctypes.byref(bi))
                assert rc == pkg._lib.MAC_E_INVAL, tag
                break
            want = -area + (viol * 1e5 if has_rmax else 0.0)
            if feas is not None:
                want = np.where(feas, want, np.inf)
            got, kern, fused = _profiled(ctx, chain, lambda: one(C, has_rmax, dl), algo="poll")
            _took(chain, kern, fused, tag)
            _check_poll(got, want, tag)


# ------------------------------------------------------------------ 5. the whole-poll rejection

@pytest.mark.parametrize("chain", ["fused", "five"])
def test_whole_poll_rejection(ctx, pkg, orc, chain):
    """The native driver at d_lim = 3 m from ell = 2 (steps of 4 m): the first polls are rejected whole
    by their prep launch (every diagonal step alone breaks cons3), the later ones, on a finer mesh, are
    not; iterate, objective and counts equal the host restatement's over the oracle's objective."""
    wl, TS, TC = pkg.workloads, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    key = ("reject",)
    if key not in _REF:
        x, y, w = wl.grid_points(64)
        rng = wl.SplitMix64(515)
        N = 12
        x0 = wl.uniform_disks(N, 64, rng, radius=20.0)
        rmax = np.full(N, 30.0 * TAN50)
        rec = recs(x, y, w)
        c3 = TC.create_cons3(x0, 100 / 180 * math.pi, np.full(N, 3.0))
        res = TS.mads(x0, lambda v: orc.ref_objective(v, rec, rmax, 1e5), [TC.cons1, c3], N_iter=10, ell0=2,
                      ell_max=6, seed=991)
        _REF[key] = dict(x=x, y=y, w=w, x0=x0, rmax=rmax, c3=c3, res=res)
    r = _REF[key]
    res, c3 = r["res"], r["c3"]
    ctx.set_points(r["x"], r["y"], r["w"])
    (xn, st), kern, fused = _profiled(
        ctx, chain, lambda: ctx.mads_run(r["x0"], r["rmax"], 1e5, prev=c3.prev, d_lim=c3.d_lim,
                                         tan_half_fov=c3.tan_half_fov, n_iter=10, ell0=2, ell_max=6, seed=991))
    assert np.array_equal(xn, res.x if res.x is not None else res.i)
    assert st["f"] == res.x_cost and st["iterations"] == res.status.iteration
    assert st["feasible_evaluations"] == res.status.cons3_passed
    assert 0 < st["rejected_polls"] <= res.status.cons3_empty_polls, st
    assert st["rejected_polls"] < st["iterations"], st
    assert ("fiw_kernel" in kern) == (chain == "fused"), kern
