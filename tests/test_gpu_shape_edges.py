"""GPU: polls on either side of every constant that routes a poll chain (tests/shape_edges.py; the
table, the shapes and the cases' teeth are checked on the CPU by tests/test_shape_edges.py).

Per case, bit for bit against the C oracle (src/AreaCoverageCalculation.jl:63-78 calculateArea,
src/TDM_STATIC_opt.jl:82-100 the objective, src/TDM_Constraints.jl:54-75 cons3): area_batch,
poll_best's objectives, argmin and best objective without and with cons3, objective_batch, and the
single-candidate area of candidate 0; on equal weights the first three through
test_gpu_parity._full_poll_check against the exact lattice count, which equals the C oracle's areas
(asserted). r_max lies inside the radius offsets' range, so the penalties are non-zero integers that
differ from row to row, zero on one row in eight. The `argmin_last` variant makes the last candidate the strict minimiser, so a
dropped last candidate shows in the argmin as well as in its own objective; the weighted variant
takes the fp64 credit rows instead of the integer counts (weights from {1, 2, 4, 8}: every partial
sum exact).

Which launches ran is read back from the profile and compared with shape_edges.route, the
restatement of eval_plan.h eval_plan's conditions: the fused chain (fiw_kernel, fin2_kernel) or
the five-launch one (disk_index_kernel, coverage_poll_kernel), or no chain at all. The roles cannot
tell the 3- from the 6-per-thread index, prep_x_kernel from prep_kernel, or a walk that leaves cons3
failures out from one that evaluates them: those are asserted on the plan itself on the CPU
(test_shape_edges.py, through mac_diag_route), and test_launch_sizes_are_the_plan_s ties the plan to
the launches by their workgroup counts; here the K (or N) on each side of the constant is what
crosses the edge.
"""
import ctypes

import numpy as np
import pytest

import shape_edges as se
from test_gpu_parity import _full_poll_check

pytestmark = pytest.mark.gpu
CHAINS = ("fused", "five")
WALKS = ("coverage_poll_kernel", "coverage_tiled_poll_kernel", "fiw_kernel")
_REF = {}


def _ref(orc, N, K, weighted=False, last=False):
    """(the case, the oracle's values of it): computed once and left unchanged."""
    key = (N, K, weighted, last)
    if key not in _REF:
        c = se.make(N, K, weighted=weighted, argmin_last=last)
        _REF[key] = (c, se.expected(orc, c))
    return _REF[key]


def _variants(orc, N, K, weighted):
    out = [_ref(orc, N, K), _ref(orc, N, K, last=True)]
    if weighted:
        out.append(_ref(orc, N, K, weighted=True))
    return out


def _routed(ctx, fn):
    """(fn's result, {launch role: launches}, the walk the profile reports) of what fn ran."""
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        out = fn()
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        walk = ctx.profile_read(reset=False)[3]
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    return out, kern, walk


def _assert_route(kern, N, K, algo, chain, fresh=False):
    runs, fiw = se.route(N, K, algo, chain, fresh)
    tag = (N, K, algo, chain, kern)
    assert any(kern.get(r, 0) for r in WALKS) == runs, tag
    if fiw is True:
        assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, tag
        assert "disk_index_kernel" not in kern and "coverage_poll_kernel" not in kern, tag
    elif fiw is False:
        assert "fiw_kernel" not in kern and "fin2_kernel" not in kern, tag
        assert (kern.get("disk_index_kernel", 0) > 0 and kern.get("coverage_poll_kernel", 0) > 0) == runs, tag
    # (fiw is None: AUTO's routing history decides)


def _check(ctx, orc, c, e, algo, tag):
    """Every device entry point of the poll against the oracle's values, under `algo`."""
    tag = (tag, algo, c.N, c.K, "weighted" if c.weighted else "equal", "last" if c.argmin_last else "")
    if not c.weighted:
        # equal weights: the areas, both polls' objectives, argmin and best objective against the
        # exact lattice count (its cons3: prev = candidate 0, d_lim = 10 m, this case's), which is
        # the C oracle's value
        assert np.all(c.d_lim == 10.0) and np.array_equal(c.prev, c.C[0])
        cnt = _full_poll_check(ctx, orc, c.C, c.r_max, c.G, [algo], str(tag))
        assert np.array_equal(25.0 * cnt.astype(np.float64), e.area), tag
        ctx.set_algo(algo)
    else:
        ctx.set_algo(algo)
        got = ctx.area_batch(c.C)
        bad = np.flatnonzero(got != e.area)
        assert bad.size == 0, (tag, "area", bad[:8], got[bad[:8]], e.area[bad[:8]])
        kw = dict(prev=c.prev, d_lim=c.d_lim, tan_half_fov=c.tan_half_fov)
        for want, k, extra in ((e.obj, e.k, {}), (e.bar, e.k_bar, kw)):
            bo, bi, objs = ctx.poll_best(c.C, c.r_max, 1e5, want_all=True, **extra)
            bad = np.flatnonzero(objs != want)
            assert bad.size == 0, (tag, "cons3" if extra else "plain", bad[:8], objs[bad[:8]], want[bad[:8]])
            assert (bi, bo) == (k, want[k]), (tag, "cons3" if extra else "plain", bi, k, bo, want[k])
    objs = ctx.objective_batch(c.C, c.r_max, 1e5)
    assert np.array_equal(objs, e.obj), (tag, "objective_batch", np.flatnonzero(objs != e.obj)[:8])
    one = ctx.area(c.C[0])
    assert one == e.area[0], (tag, "area of candidate 0", one, e.area[0])


def _reset(ctx):
    ctx.set_algo("auto")
    ctx.set_chain("auto")
    ctx.profile(False)


def _forced(ctx, orc, N, K, weighted, chain, algo="auto"):
    """The case's variants under one forced chain; the route of each variant's first batch."""
    try:
        for c, e in _variants(orc, N, K, weighted):
            ctx.set_points(c.x, c.y, c.w)
            ctx.set_chain(chain)
            ctx.set_algo(algo)
            got, kern, _ = _routed(ctx, lambda: ctx.area_batch(c.C))
            assert np.array_equal(got, e.area), (N, K, chain, np.flatnonzero(got != e.area)[:8])
            _assert_route(kern, N, K, algo, chain)
            _check(ctx, orc, c, e, algo, chain)
    finally:
        _reset(ctx)


def _auto(pkg, orc, N, K, weighted):
    """The same on a fresh context under AUTO (the routing history belongs to the context): the
    route of its first poll, then every variant."""
    with pkg.Context(0) as c2:
        first = True
        for c, e in _variants(orc, N, K, weighted):
            c2.set_points(c.x, c.y, c.w)
            got, kern, _ = _routed(c2, lambda: c2.area_batch(c.C))
            assert np.array_equal(got, e.area), (N, K, "auto", np.flatnonzero(got != e.area)[:8])
            _assert_route(kern, N, K, "auto", "auto", fresh=first)
            first = False
            _check(c2, orc, c, e, "auto", "auto")


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("K", [k for k, _ in se.K_EDGES])
def test_k_edges_forced_chain(ctx, orc, K, chain):
    """N = 8, K on each side of kPollMinK, kFwMaxK + 1 (= kIndexMaxK + 1) and kIndexMaxKWide + 1, and
    the remainders 2, 3, 4 of K mod kPrepCX: fiw_kernel runs at 64, 65, 3072, 3073 and the remainder
    cases when forced, at none of them under "five", and neither at 63 (no chain) nor from 3074 on
    (disk_index_kernel instead), whatever is forced."""
    _forced(ctx, orc, se.N_K, K, K in se.K_WEIGHTED, chain)


@pytest.mark.parametrize("K", [k for k, _ in se.K_EDGES])
def test_k_edges_auto(pkg, orc, K):
    """AUTO on a fresh context: its first poll takes the fused chain from kPollMinK to kFwMaxK + 1
    (8 disks cannot seed the history as crowded), no chain at 63, the five-launch one above."""
    _auto(pkg, orc, se.N_K, K, K in se.K_WEIGHTED)


def _role_slots(pkg, ctx):
    """{launch role: workgroups that took stamps} of the launches recorded since the last reset
    (the host-only mac_diag_role_slots)."""
    L = ctx._L
    L.mac_diag_role_slots.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.mac_diag_role_slots.restype = ctypes.c_int32
    roles = pkg._lib.PROF_ROLES
    out = (ctypes.c_int64 * len(roles))()
    assert L.mac_diag_role_slots(ctx._h, out, len(roles)) == 0
    return {name: int(out[r]) for r, name in enumerate(roles)}


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("K", [63, 64, 3073, 3074, 6146])
def test_launch_sizes_are_the_plan_s(pkg, ctx, orc, K, chain):
    """The route plan (eval_plan through mac_diag_route, asserted against the table on the CPU) is what
    was launched: the workgroups of the chain's first, index / fiw_kernel and last launch."""
    N = se.N_K
    c, e = _ref(orc, N, K)
    try:
        ctx.set_points(c.x, c.y, c.w)
        ctx.set_chain(chain)
        ctx.profile(True)
        ctx.profile_read(reset=True)
        got = ctx.area_batch(c.C)
        slots = _role_slots(pkg, ctx)
    finally:
        ctx.profile_read(reset=True)
        _reset(ctx)
    assert np.array_equal(got, e.area)
    p = se.plan(N, K, "auto", chain, want_area=True, want_obj=False, M=c.x.size, w_uniform=True)
    if p.fused_eligible:      # (forced: the routing history has no say)
        want = {"prep_kernel": p.nprep, "fiw_kernel": p.nfw, "fin2_kernel": p.nfin2}
    elif p.poll_possible:
        want = {"prep_kernel": p.nrec, "disk_index_kernel": p.nidx, "finalize_kernel": p.nfin}
    else:
        want = {}
    assert bool(p.fused_eligible) == (chain == "fused" and 64 <= K <= 3073), (K, chain)
    for role in ("prep_kernel", "disk_index_kernel", "finalize_kernel", "fiw_kernel", "fin2_kernel"):
        assert slots[role] == want.get(role, 0), (K, chain, role, slots, vars(p))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("N", [n for n, _ in se.N_EDGES])
def test_n_edges_forced_chain(ctx, orc, N, chain):
    """K = 70, N = 1, 2, 7, 8, 9 (idle workgroups of the 8-aligned launches), 511, 512, 513 (kPrepU:
    the prep's layout, cons3 failures left out or evaluated, one or two UAV blocks) and 2048, 2049
    (kTiledMaxN)."""
    _forced(ctx, orc, N, se.K_FOR_N, N in se.N_WEIGHTED, chain)


@pytest.mark.parametrize("N", [n for n, _ in se.N_EDGES])
def test_n_edges_auto(pkg, orc, N):
    _auto(pkg, orc, N, se.K_FOR_N, N in se.N_WEIGHTED)


@pytest.mark.parametrize("N", [se.kTiledMaxN, se.kTiledMaxN + 1])
def test_tiled_option_at_the_lds_limit(ctx, orc, N):
    """algo="tiled" is honoured at N = kTiledMaxN (the per-candidate walk inside the five-launch
    chain) and becomes the poll walk one disk above; the values stay the oracle's."""
    c, e = _ref(orc, N, se.K_FOR_N)
    try:
        ctx.set_points(c.x, c.y, c.w)
        ctx.set_algo("tiled")
        got, kern, walk = _routed(ctx, lambda: ctx.area_batch(c.C))
        assert np.array_equal(got, e.area), np.flatnonzero(got != e.area)[:8]
        if N <= se.kTiledMaxN:
            assert walk == "tiled" and kern.get("coverage_tiled_poll_kernel", 0) > 0, (walk, kern)
            assert "fiw_kernel" not in kern, kern
        else:
            assert walk == "poll" and "coverage_tiled_poll_kernel" not in kern, (walk, kern)
        _check(ctx, orc, c, e, "tiled", "auto")
    finally:
        _reset(ctx)


@pytest.mark.parametrize("chain", CHAINS)
def test_small_k_through_the_chains(ctx, orc, chain):
    """K = 1 .. 36 at N = 8 with the poll walk forced, the only way into the chains below kPollMinK:
    every flip between prep_x_kernel and prep_kernel, and blocks of the prep and of fin2 that are
    not full. One list for all 36 polls."""
    x, y, w = se.points(se.grid_size(se.N_K), False, 1)
    try:
        ctx.set_points(x, y, w)
        ctx.set_chain(chain)
        for K in se.SMALL_K:
            for last in (False, True):
                c, e = _ref(orc, se.N_K, K, last=last)
                assert c.x is x
                ctx.set_algo("poll")
                got, kern, walk = _routed(ctx, lambda: ctx.area_batch(c.C))
                assert np.array_equal(got, e.area), (K, chain, got, e.area)
                assert walk == "poll", (K, walk)
                _assert_route(kern, se.N_K, K, "poll", chain)
                _check(ctx, orc, c, e, "poll", chain)
    finally:
        _reset(ctx)


@pytest.mark.parametrize("N", [n for n, _ in se.GEN_N])
def test_basis_form_prep_layouts(ctx, orc, N):
    """Basis-form polls (K = 6N, mesh step 8) through the three generated-source prep layouts side
    by side (gen_x: N <= kPrepU; pair: 3N a multiple of 4; else prep_kernel by candidates), under
    each chain, without and with cons3: the objectives equal the matrix poll's on the matrix the same
    products build and -25 x the exact lattice count + 1e5 x the violation, the argmin is the lowest
    minimiser. (The layouts share the prep's launch role: no route is asserted beyond the chain.)"""
    c = se.make_gen(N)
    e = se.expected(orc, c, exact=False)
    kw = dict(prev=c.prev, d_lim=c.d_lim, tan_half_fov=c.tan_half_fov)
    try:
        ctx.set_points(c.x, c.y, c.w)
        for chain in ("auto",) + CHAINS:
            ctx.set_chain(chain)
            for want, k, extra in ((e.obj, e.k, {}), (e.bar, e.k_bar, kw)):
                (bo, bi, objs), kern, _ = _routed(ctx, lambda: ctx.poll_basis(
                    c.x0, c.L, c.rp, c.cp, c.delta, c.r_max, 1e5, want_all=True, **extra))
                tag = (N, chain, bool(extra))
                bad = np.flatnonzero(objs != want)
                assert bad.size == 0, (tag, bad[:8], objs[bad[:8]], want[bad[:8]])
                assert (bi, bo) == (k, want[k]), (tag, bi, k, bo, want[k])
                if chain != "auto":    # (AUTO: the history and the host's crowding estimate decide)
                    _assert_route(kern, N, c.K, "auto", chain)
                mo, mi, mobjs = ctx.poll_best(c.C, c.r_max, 1e5, want_all=True, **extra)
                assert np.array_equal(mobjs, want) and (mi, mo) == (k, want[k]), tag
    finally:
        _reset(ctx)
