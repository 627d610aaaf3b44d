"""GPU: the coverage predicate at the ulp boundary on every device path.

The cases (tests/boundary_cases.py; tests/test_boundary_cases.py checks them on the CPU) hold entries
with a == T(r) ("on": covered) and a == next_up(T(r)) ("off": not covered) for the disks of the
poll's own candidates, a ladder of a - T across the fp32 filter's band edge, and real-valued
incumbents whose on-mesh moves pack into key words. Every expected value is the C oracle's
(src/AreaCoverageCalculation.jl:63-78 calculateArea, src/TDM_STATIC_opt.jl:82-100 the objective,
src/TDM_Constraints.jl:54-75 cons3, src/CellFunctions.jl:81-108 rmvCoveredPOI) or the numpy
restatement's per-entry flags, never another device path's; everything is exact equality (the
"pow2" weights make every partial sum exact, so the fp64 credit paths are compared bit for bit).

A mismatch reports the entries the device decided differently, with their class and targeted disk
(`_explain`), through covered_flags of the candidate.

Nothing here runs the f32 caller path: fp32 coordinates cannot be placed within ulps of an fp64
threshold, and after their exact widening they run the same kernels.
"""
import numpy as np
import pytest

import boundary_cases as bc
from test_gpu_bydisk import np_by_disk

pytestmark = pytest.mark.gpu
_REF = {}


def _recs(x, y, w):
    return np.stack([x, y, w, w, np.zeros_like(x)], axis=1)


def _ref(name, weights, orc):
    """(the case, the oracle's values of it): computed once and left unchanged."""
    key = (name, weights)
    c = bc.make_case(name, weights)
    if key not in _REF:
        rec = _recs(c.x, c.y, c.w)
        area = orc.PointerList(rec).area_batch(c.C)
        obj = -area + orc.violation_batch(c.C, c.r_max) * 1e5
        feas = orc.cons3_batch(c.prev, c.C, c.d_lim, bc.TAN50)
        kept = orc.ref_remove_covered(c.C[0], rec)
        area_kept = orc.PointerList(rec[kept]).area_batch(c.C)
        for a in (rec, area, obj, feas, kept, area_kept):
            a.setflags(write=False)
        _REF[key] = dict(rec=rec, area=area, obj=obj, feas=feas, kept=kept, area_kept=area_kept)
    return c, _REF[key]


def _explain(c, got, want):
    """The entries decided differently: (entry, class, targeted disk, miss / false hit)."""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return [(int(e), bc.CLASS_NAMES[int(c.cls[e])],
             tuple(c.disks[c.disk[e]]) if c.disk[e] >= 0 else None,
             "miss" if want[e] else "false hit") for e in bad[:8]], bad.size


def _why(ctx, orc, c, k):
    """For a failed area of candidate k: what covered_flags decides differently from the oracle."""
    return _explain(c, ctx.covered_flags(c.C[k]), orc.np_covered(c.C[k], c.x, c.y))


def _profiled(ctx, fn):
    """(fn's result, {launch role: launches}) of the poll chains fn ran."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        out = fn()
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    return out, kern


@pytest.fixture
def case(request, ctx, orc):
    name, weights = request.param
    c, ref = _ref(name, weights, orc)
    ctx.set_points(c.x, c.y, c.w)
    try:
        yield c, ref
    finally:
        ctx.set_algo("auto")
        ctx.set_shared("auto")
        ctx.set_chain("auto")
        ctx.profile(False)


def _params(names=bc.CASES):
    return [pytest.param((n, w), id=f"{n}-{w}") for n in names for w in bc.WEIGHTS]


@pytest.mark.parametrize("case", _params(), indirect=True)
def test_single_candidate_paths(ctx, orc, case):
    """Row 0 and the two corner rows, one candidate at a time: the closure kernel's area under every
    algorithm option, the per-entry flags (a miss and a false hit cannot cancel), and the per-disk
    attribution, where boundary entries of a higher disk lie inside lower disks' boxes and the
    other way round, so both neighbour sides decide at the threshold."""
    c, ref = case
    for k in (0, c.row_in, c.row_out):
        cand = c.C[k]
        want_flags = orc.np_covered(cand, c.x, c.y)
        got_flags = ctx.covered_flags(cand)
        assert np.array_equal(got_flags, want_flags), (c.name, k, _explain(c, got_flags, want_flags))
        for algo in ("auto", "tiled", "scan", "poll"):
            ctx.set_algo(algo)
            got = ctx.area(cand)
            assert got == ref["area"][k], (c.name, c.weights, k, algo, got, ref["area"][k])
        ctx.set_algo("auto")
        owned, excl, area = ctx.area_by_disk(cand)
        wo, wx, wa = np_by_disk(orc, cand, c.x, c.y, c.w)
        assert wa == ref["area"][k]
        assert np.array_equal(owned, wo), (c.name, k, "owned", np.flatnonzero(owned != wo), owned - wo)
        assert np.array_equal(excl, wx), (c.name, k, "exclusive", np.flatnonzero(excl != wx), excl - wx)
        assert area == wa, (c.name, k, area, wa)


# (algorithm, chain, shared-entry mode)
BATCH_PATHS = [("tiled", "auto", "auto"), ("scan", "auto", "auto"), ("poll", "five", "auto"),
               ("poll", "five", "fp64"), ("poll", "five", "bits"), ("poll", "fused", "auto"),
               ("auto", "auto", "auto")]


@pytest.mark.parametrize("case", _params(), indirect=True)
def test_batch_paths(ctx, orc, case):
    """area_batch of the whole poll through the per-candidate walk, the scan, the five-launch chain
    under each shared-entry mode, the fused chain, and everything on auto; the launches that ran are
    read back from the profile."""
    c, ref = case
    for algo, chain, shared in BATCH_PATHS:
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        ctx.set_shared(shared)
        first = ctx.area_batch(c.C)     # (also the shared-entry pass's launch hint for the second)
        got, kern = _profiled(ctx, lambda: ctx.area_batch(c.C))
        print(f"{c.name}/{c.weights} {algo}/{chain}/{shared}: {kern}")
        for g in (first, got):
            bad = np.flatnonzero(g != ref["area"])
            assert bad.size == 0, (c.name, c.weights, algo, chain, shared, bad[:8], g[bad[:8]],
                                   ref["area"][bad[:8]], _why(ctx, orc, c, int(bad[0])))
        if chain == "fused" and c.name in ("near", "far", "big"):
            assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern
        if chain == "five":
            assert "fiw_kernel" not in kern and kern.get("coverage_poll_kernel", 0) > 0, kern
        if (chain, shared) == ("five", "auto") and c.name == "crowded" and c.weights == "equal":
            # the union pass is launched on a hint, the lane's earlier polls' count of disks with
            # neighbours, and the context's lanes take turns: a run of polls, so that one of them
            # follows a crowded poll on its own lane
            outs, kern = _profiled(ctx, lambda: [ctx.area_batch(c.C) for _ in range(12)])
            print(f"{c.name}/{c.weights} {algo}/{chain}/{shared} x 12: {kern}")
            assert all(np.array_equal(g, ref["area"]) for g in outs)
            assert kern.get("shared_or_kernel", 0) > 0, kern


@pytest.mark.parametrize("case", _params(), indirect=True)
def test_poll_best_with_and_without_cons3(ctx, orc, case):
    """The poll's objectives and argmin, bit for bit, with a cons3 limit that fails some candidates
    and keeps others: failed candidates are left out of the regions and the displacement bound, so
    other entries reach the annulus shortcut and other ones the tests."""
    c, ref = case
    feas = ref["feas"]
    assert 0 < int(feas.sum()) < c.K
    kw = dict(prev=c.prev, d_lim=c.d_lim, tan_half_fov=bc.TAN50)
    for algo, chain in (("poll", "five"), ("poll", "fused"), ("auto", "auto")):
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        for cons3 in (True, False):
            want = np.where(feas, ref["obj"], np.inf) if cons3 else ref["obj"]
            bo, bi, objs = ctx.poll_best(c.C, c.r_max, 1e5, want_all=True, **(kw if cons3 else {}))
            bad = np.flatnonzero(objs != want)
            assert bad.size == 0, (c.name, c.weights, algo, chain, cons3, bad[:8], objs[bad[:8]],
                                   want[bad[:8]], _why(ctx, orc, c, int(bad[0])))
            k = int(np.argmin(want))
            assert (bi, bo) == (k, want[k]), (c.name, algo, chain, cons3, bi, k, bo, want[k])


@pytest.mark.parametrize("case", _params(["near"]), indirect=True)
def test_poll_basis_form(ctx, orc, case):
    """The same poll in basis form (L's triangle, its permutations and delta, expanded on the
    device): the expansion reproduces C[1:1 + 2n] bit for bit, and the results equal the matrix
    poll's and the oracle's, with and without cons3. (The corner rows are no LTMADS directions:
    they follow the 2n rows of the poll.)"""
    c, ref = case
    Lm, rp, cp, delta = c.basis
    n = 3 * c.N
    assert c.n_poll == 2 * n
    B = Lm[rp][:, cp].astype(np.float64)
    P = np.ascontiguousarray(np.concatenate([c.C[0][None, :] + delta * B.T, c.C[0][None, :] - delta * B.T]))
    assert np.array_equal(P.view(np.uint64), c.C[1:1 + 2 * n].view(np.uint64))
    kw = dict(prev=c.prev, d_lim=c.d_lim, tan_half_fov=bc.TAN50)
    for chain in ("auto", "five", "fused"):
        ctx.set_chain(chain)
        for cons3 in (True, False):
            want = ref["obj"][1:1 + 2 * n]
            if cons3:
                want = np.where(ref["feas"][1:1 + 2 * n], want, np.inf)
            bo, bi, objs = ctx.poll_basis(c.C[0], Lm, rp, cp, delta, c.r_max, 1e5, want_all=True,
                                          **(kw if cons3 else {}))
            mo, mi, mobjs = ctx.poll_best(P, c.r_max, 1e5, want_all=True, **(kw if cons3 else {}))
            bad = np.flatnonzero(objs != want)
            assert bad.size == 0, (chain, cons3, bad[:8], objs[bad[:8]], want[bad[:8]],
                                   _why(ctx, orc, c, 1 + int(bad[0])))
            assert np.array_equal(mobjs, want), (chain, cons3)
            k = int(np.argmin(want))
            assert (bi, bo) == (k, want[k]) == (mi, mo), (chain, cons3, bi, mi, k)


@pytest.mark.parametrize("case", _params(), indirect=True)
def test_list_maintenance(ctx, orc, case):
    """remove_covered under the incumbent: the oracle's kept indices (the on entries of candidate
    0's disks go, its decisive off entries stay), the kept list itself, and on the rebuilt index
    the poll's areas (the targeted rows among them) against the oracle on the kept list."""
    c, ref = case
    kept = ctx.remove_covered(c.C[0])
    want = ref["kept"]
    flags = np.ones(c.x.size, dtype=bool)
    flags[kept] = False
    want_flags = np.ones(c.x.size, dtype=bool)
    want_flags[want] = False
    assert np.array_equal(kept, want), (c.name, _explain(c, flags, want_flags))
    mine = np.isin(c.disk, c.disk_of[0])
    on, off = mine & (c.cls == bc.ON), mine & (c.cls == bc.OFF)
    assert on.sum() >= c.need * c.exposed[0].sum() and not np.isin(np.flatnonzero(on), kept).any()
    assert np.isin(np.flatnonzero(off), kept).sum() >= c.need * c.exposed[0].sum()
    gx, gy, gw = ctx.get_points()
    assert np.array_equal(gx, c.x[want]) and np.array_equal(gy, c.y[want]) and np.array_equal(gw, c.w[want])
    for algo, chain in (("auto", "auto"), ("poll", "five"), ("poll", "fused"), ("tiled", "auto")):
        ctx.set_algo(algo)
        ctx.set_chain(chain)
        got = ctx.area_batch(c.C)      # (the whole poll: the chains need K >= 64)
        bad = np.flatnonzero(got != ref["area_kept"])
        assert bad.size == 0, (c.name, c.weights, algo, chain, bad[:8], np.isin(bad, c.rows)[:8])
    assert not np.array_equal(ref["area_kept"][c.rows], ref["area"][c.rows])
