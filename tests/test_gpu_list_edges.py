"""GPU: every consumer of the tile index on lists at its edges (tests/list_cases.py; the cases are
checked on the CPU by tests/test_list_cases.py).

The closure kernel, coverage_tiled_kernel, the five-launch chain and its shared-entry passes, the
fused chain (fiw_kernel, fin2_kernel), by_disk_kernel, the region-stats kernel and
covered_flags_tiled_kernel all read the list through build_index's bounding box, grid, keys, sorted
copy and offsets. Every expected value here is the oracle's (src/AreaCoverageCalculation.jl:63-78
calculateArea, src/TDM_STATIC_opt.jl:82-100 the objective, src/TDM_Constraints.jl:54-75 cons3,
src/CellFunctions.jl:81-108 rmvCoveredPOI) or a numpy restatement's, never another device path's,
and every comparison is exact: weights are 25 or distinct powers of two.

A mismatch reports the entries the device decided differently, with their coordinates and what
they are to the index (`_explain`), through covered_flags of the candidate.
"""
import numpy as np
import pytest

import list_cases as lc
from test_gpu_boundary import BATCH_PATHS, _profiled
from test_gpu_bydisk import np_by_disk
from test_gpu_regions import _assert_stats, _expect_stats

pytestmark = pytest.mark.gpu
_REF = {}
FULL = [n for n in lc.CASES if n != "wide_grid_stride"]     # (the largest list: flags and one poll)


def _same(a, b):
    """Bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _ref_of(key, x, y, w, C, r_max, prev, d_lim, orc, light=False):
    """The oracle's values of a list and its poll: computed once and left unchanged."""
    if key not in _REF:
        rec = lc.recs(x, y, w)
        ref = dict(rec=rec, area=orc.PointerList(rec).area_batch(C))
        if not light:
            ref["obj"] = -ref["area"] + orc.violation_batch(C, r_max) * 1e5
            ref["feas"] = orc.cons3_batch(prev, C, d_lim, lc.TAN50)
            ref["kept"] = orc.ref_remove_covered(C[0], rec)
            ref["area_kept"] = orc.PointerList(rec[ref["kept"]]).area_batch(C)
        for a in ref.values():
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _ref(name, orc):
    c = lc.make_case(name)
    return c, _ref_of(name, c.x, c.y, c.w, c.C, c.r_max, c.prev, c.d_lim, orc, c.light)


def _classes(x, y):
    """Per entry, what it is to the index: non-finite (keyed to tile 0 / the last tile), on the
    bounding box, one of several at its position, or plain."""
    xmn, xmx, ymn, ymx = lc.finite_bbox(x, y)
    _, inv, cnt = np.unique(np.stack([x, y], axis=1), axis=0, return_inverse=True, return_counts=True)
    out = np.full(x.size, "plain", dtype=object)
    out[cnt[inv.ravel()] > 1] = "duplicate"
    out[(x == xmn) | (x == xmx) | (y == ymn) | (y == ymx)] = "on the bounding box"
    out[~(np.isfinite(x) & np.isfinite(y))] = "non-finite"
    return out


def _explain(x, y, got, want):
    """The entries decided differently: (entry, x, y, class, miss / false hit)."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    cls = _classes(x, y)
    return [(int(e), float(x[e]), float(y[e]), cls[e], "miss" if want[e] else "false hit")
            for e in bad[:8]], bad.size


def _why(ctx, orc, x, y, cand):
    return _explain(x, y, ctx.covered_flags(cand), orc.np_covered(cand, x, y))


def _reset(ctx):
    ctx.set_algo("auto")
    ctx.set_shared("auto")
    ctx.set_chain("auto")
    ctx.profile(False)
    ctx.clear_regions()


@pytest.fixture
def case(request, ctx, orc):
    c, ref = _ref(request.param, orc)
    ctx.set_points(c.x, c.y, c.w)
    try:
        yield c, ref
    finally:
        _reset(ctx)


def _check_batch_paths(ctx, orc, tag, x, y, C, want, must_fuse):
    for algo, chain, shared in BATCH_PATHS:
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        ctx.set_shared(shared)
        first = ctx.area_batch(C)       # (also the shared-entry pass's launch hint for the second)
        got, kern = _profiled(ctx, lambda: ctx.area_batch(C))
        print(f"{tag} {algo}/{chain}/{shared}: {kern}")
        for g in (first, got):
            bad = np.flatnonzero(g != want)
            assert bad.size == 0, (tag, algo, chain, shared, bad[:8], g[bad[:8]], want[bad[:8]],
                                   _why(ctx, orc, x, y, C[int(bad[0])]))
        if chain == "fused" and must_fuse:
            assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, (tag, kern)
        if chain == "five":
            assert "fiw_kernel" not in kern and kern.get("coverage_poll_kernel", 0) > 0, (tag, kern)


def _check_poll_best(ctx, orc, tag, x, y, C, r_max, prev, d_lim, ref, both=True):
    feas = ref["feas"]
    assert 0 < int(feas.sum()) < C.shape[0]
    kw = dict(prev=prev, d_lim=d_lim, tan_half_fov=lc.TAN50)
    for algo, chain in (("poll", "five"), ("poll", "fused"), ("auto", "auto")):
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        for cons3 in ((True, False) if both else (True,)):
            want = np.where(feas, ref["obj"], np.inf) if cons3 else ref["obj"]
            bo, bi, objs = ctx.poll_best(C, r_max, 1e5, want_all=True, **(kw if cons3 else {}))
            bad = np.flatnonzero(objs != want)
            assert bad.size == 0, (tag, algo, chain, cons3, bad[:8], objs[bad[:8]], want[bad[:8]],
                                   _why(ctx, orc, x, y, C[int(bad[0])]))
            k = int(np.argmin(want))
            assert (bi, bo) == (k, want[k]), (tag, algo, chain, cons3, bi, k, bo, want[k])


def _check_by_disk(ctx, orc, tag, x, y, w, cand, want_area):
    owned, excl, area = ctx.area_by_disk(cand)
    wo, wx, wa = np_by_disk(orc, cand, x, y, w)
    assert wa == want_area
    assert np.array_equal(owned, wo), (tag, "owned", np.flatnonzero(owned != wo), owned - wo)
    assert np.array_equal(excl, wx), (tag, "exclusive", np.flatnonzero(excl != wx), excl - wx)
    assert area == wa, (tag, area, wa)
    return owned, excl


def _check_removal(ctx, orc, tag, x, y, w, C, ref):
    kept = ctx.remove_covered(C[0])
    want = ref["kept"]
    got_flags, want_flags = np.ones(x.size, dtype=bool), np.ones(x.size, dtype=bool)
    got_flags[kept] = False
    want_flags[want] = False
    assert np.array_equal(kept, want), (tag, _explain(x, y, got_flags, want_flags))
    assert ctx.num_points == want.size
    gx, gy, gw = ctx.get_points()
    assert _same(gx, x[want]) and _same(gy, y[want]) and _same(gw, w[want]), tag
    for algo, chain in (("auto", "auto"), ("poll", "five"), ("poll", "fused"), ("tiled", "auto")):
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        got = ctx.area_batch(C)
        bad = np.flatnonzero(got != ref["area_kept"])
        assert bad.size == 0, (tag, algo, chain, bad[:8], got[bad[:8]], ref["area_kept"][bad[:8]],
                               _why(ctx, orc, x[want], y[want], C[int(bad[0])]))


# ---- every case on the session's context ---------------------------------------------------------

@pytest.mark.parametrize("case", lc.CASES, indirect=True)
def test_set_points_and_flags(ctx, orc, case):
    """The list goes in and comes back bit for bit, and the per-entry flags of the incumbent and two
    more candidates are the oracle's: a miss and a false hit cannot cancel."""
    c, ref = case
    assert ctx.num_points == c.x.size
    gx, gy, gw = ctx.get_points()
    assert _same(gx, c.x) and _same(gy, c.y) and _same(gw, c.w)
    for k in c.flag_rows:
        want = orc.np_covered(c.C[k], c.x, c.y)
        got = ctx.covered_flags(c.C[k])
        assert np.array_equal(got, want), (c.name, k, _explain(c.x, c.y, got, want))
        if not c.light:
            for algo in ("auto", "tiled", "scan", "poll", "poll", "poll", "poll"):
                # (the poll chain four times: the context's lanes take turns, each with scratch of
                # its own)
                ctx.set_algo(algo)
                got = ctx.area(c.C[k])
                assert got == ref["area"][k], (c.name, k, algo, got, ref["area"][k])
            ctx.set_algo("auto")


@pytest.mark.parametrize("case", lc.CASES, indirect=True)
def test_batch_paths(ctx, orc, case):
    """area_batch of the poll through the per-candidate walk, the scan, the five-launch chain under
    each shared-entry mode, the fused chain and auto, each twice (the second follows the first's
    hint); the launches that ran are read back and printed."""
    c, ref = case
    _check_batch_paths(ctx, orc, c.name, c.x, c.y, c.C, ref["area"], c.name in lc.FUSED)


@pytest.mark.parametrize("name", ["outlier", "outlier_1e30", "span_overflow_xy", "heavy_tile"])
def test_batch_paths_weighted(ctx, pkg, orc, name):
    """The same lists with weights from {1, 2, 4, 8} (every sum exact): the f64 credit rows, and
    under shared = bits the bit-word kernel in place of the union pass."""
    c = lc.make_case(name)
    w = 2.0 ** pkg.workloads.SplitMix64(31 + len(name)).integers(0, 3, c.x.size).astype(np.float64)
    ref = _ref_of(("pow2", name), c.x, c.y, w, c.C, c.r_max, c.prev, c.d_lim, orc, light=True)
    assert np.unique(ref["area"]).size > 8
    try:
        ctx.set_points(c.x, c.y, w)
        _check_batch_paths(ctx, orc, name + "/pow2", c.x, c.y, c.C, ref["area"], name in lc.FUSED)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("case", FULL, indirect=True)
def test_poll_best_with_and_without_cons3(ctx, orc, case):
    c, ref = case
    _check_poll_best(ctx, orc, c.name, c.x, c.y, c.C, c.r_max, c.prev, c.d_lim, ref)


@pytest.mark.parametrize("case", FULL, indirect=True)
def test_attribution_and_region_stats(ctx, orc, case):
    """area_by_disk of the incumbent, then the region stats under a populated and an empty box
    (w_high = NaN: the weights stay)."""
    c, ref = case
    owned, _ = _check_by_disk(ctx, orc, c.name, c.x, c.y, c.w, c.C[0], ref["area"][0])
    if c.name == "heavy_tile":
        # the 3,001 entries of the heavy tile lie inside disks 3 and 7: disk 3 owns them, once
        heavy = 3001 * 25.0
        assert owned[3] >= heavy and owned[7] < heavy and (owned >= heavy).sum() == 1
    x_lo, x_hi, y_lo, y_hi = c.box
    xm, ym = 0.5 * (x_lo + x_hi), 0.5 * (y_lo + y_hi)
    boxes = ([x_lo, xm], [x_hi, xm], [y_lo, ym], [y_hi, ym])
    ctx.set_regions(*boxes)
    want = _expect_stats(c.x, c.y, c.w, boxes, c.C[0], orc)
    assert want["box_count"][0] > 0 and want["box_count"][1] == 0
    _assert_stats(ctx.region_stats(c.C[0]), want, where=c.name)
    ctx.clear_regions()
    gx, gy, gw = ctx.get_points()
    assert _same(gw, c.w)


@pytest.mark.parametrize("case", FULL, indirect=True)
def test_removal_and_rebuild(ctx, orc, case):
    """remove_covered under the incumbent, then the poll on the rebuilt index."""
    c, ref = case
    _check_removal(ctx, orc, c.name, c.x, c.y, c.w, c.C, ref)


# ---- tile_points = 1, 4, 4096 in contexts of their own -------------------------------------------

def _tile_list(name, pkg):
    """(x, y, w, C, r_max, prev, d_lim) of the lists run under every tile_points setting."""
    if name == "heavy_tile":
        c = lc.make_case(name)
        return c.x, c.y, c.w, c.C, c.r_max, c.prev, c.d_lim
    # lattice48: 48 x 48 entries. lattice24x96: the same M, 96 entries tall, so that tile_points = 1
    # gives 96 tile rows and the r = 170 disk spans more than kPollRB = 64 of them (a 48 x 48 lattice
    # has 48 rows at the most).
    n, m = (48, 48) if name == "lattice48" else (24, 96)
    x, y = lc.lattice(n, 5.0, m=m)
    rng = pkg.workloads.SplitMix64(4800 + n)
    x0 = lc._disks(rng, 10, 5 * n - 10, 10, 5 * m - 10, 14, 26)
    # (beside the square lattice, which it would otherwise cover whole; across the tall one)
    x0[[4, lc.N + 4, 2 * lc.N + 4]] = (-60.0 if n == m else 5 * n // 2, 5 * m // 2, 170.0)
    C = lc._poll(x0, rng)
    return (x, y, np.full(x.size, 25.0), C, np.full(lc.N, 30.0 * lc.TAN50), x0,
            np.full(lc.N, lc.cons3_limit(C, x0)))


@pytest.mark.parametrize("tile_points", [1, 4, 4096])
@pytest.mark.parametrize("name", ["lattice48", "lattice24x96", "heavy_tile"])
def test_tile_points(pkg, orc, name, tile_points):
    """One entry per tile (the r = 170 disk spans every tile row), the default, and the whole list
    in one tile: the same paths, poll_best with cons3, the attribution, removal and rebuild."""
    x, y, w, C, r_max, prev, d_lim = _tile_list(name, pkg)
    ref = _ref_of(("tile", name), x, y, w, C, r_max, prev, d_lim, orc)
    n_cov = ref["area"] / 25.0
    assert np.unique(n_cov).size > 8 and 0 < n_cov.min() and n_cov.max() < x.size
    assert 0 < ref["kept"].size < x.size
    tag = f"{name}/tile_points={tile_points}"
    with pkg.Context(0, tile_points=tile_points) as c:
        c.set_points(x, y, w)
        _check_batch_paths(c, orc, tag, x, y, C, ref["area"], False)
        _check_poll_best(c, orc, tag, x, y, C, r_max, prev, d_lim, ref, both=False)
        c.set_algo("auto")
        c.set_chain("auto")
        _check_by_disk(c, orc, tag, x, y, w, C[0], ref["area"][0])
        _check_removal(c, orc, tag, x, y, w, C, ref)
