"""GPU: crowded polls on either side of every chunk constant of the shared-entry passes (tests/
crowded_cases.py; the table, the shapes and the cases' teeth are checked on the CPU by tests/
test_crowded_cases.py).

Every case goes through the forced poll walk on the forced five-launch chain under each forced
shared-entry mode, on the equal-weight list (integer count rows; "bits" = the union pass,
shared_or_kernel) and on the weighted one (fp64 rows; "bits" = the bit-word kernel,
shared_bits_kernel<false>), bit for bit against the C oracle (src/AreaCoverageCalculation.jl:63-78
calculateArea, src/TDM_STATIC_opt.jl:82-100 the objective, src/TDM_Constraints.jl:54-75 cons3):
area_batch, and poll_best's objectives, argmin and best objective, each twice on a context of its own
(the first poll's walk grid has one row of position slices, so the slice loop runs ceil(U / kPollKPB)
times; a later poll may take up to POLL_ROWS rows from the first's hint).

The launch roles cannot tell a shared-entry pass that ran from one that stood down (the kernel is
launched either way and returns at once), so what decided the shared entries is read back with the
host-only mac_diag_poll_report: the counters walk_setup_kernel left, from which k_or.h shared_route is
restated (crowded_cases.shared_route), and the index's positions per disk, which must equal the
generator's targets."""
import ctypes

import numpy as np
import pytest

import crowded_cases as cc

pytestmark = pytest.mark.gpu
BITS_ON = {"fp64": 0, "bits": 2}      # maxcover.hip shared_pass_hint under a forced mode
_REF = {}


def _ref(orc, name, variant="", weighted=False):
    """(the case, the oracle's values of it): computed once and left unchanged."""
    key = (name, variant, weighted)
    if key not in _REF:
        c = cc.make_u16() if name == "u16" else cc.make(name, variant)
        _REF[key] = (c, cc.expected(orc, c, weighted))
    return _REF[key]


def _role_slots(pkg, ctx):
    L = ctx._L
    L.mac_diag_role_slots.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.mac_diag_role_slots.restype = ctypes.c_int32
    roles = pkg._lib.PROF_ROLES
    out = (ctypes.c_int64 * len(roles))()
    assert L.mac_diag_role_slots(ctx._h, out, len(roles)) == 0
    return {name: int(out[r]) for r, name in enumerate(roles)}


def _expected_route(c, weighted, shared):
    """(route, counters) the case must show under a forced mode: 0 the poll kernel's fp64 jobs, 1 the
    bit-word kernel, 2 the union pass."""
    bits_on, counts = BITS_ON[shared], 0 if weighted else 1
    want = cc.counters(c, union_setup=bool(bits_on and counts))
    return cc.shared_route(want, bits_on, counts), want


def _assert_report(rep, c, weighted, shared, tag, ucount=True):
    route, want = _expected_route(c, weighted, shared)
    assert rep["walk"] == "poll", (tag, rep)
    got = {k: rep[k] for k in want}
    assert got == want, (tag, got, want)
    assert cc.shared_route(rep, BITS_ON[shared], 0 if weighted else 1) == route, (tag, rep)
    jobs = sum(rep[f"or_jobs{b}"] for b in range(4))
    if route == 2:      # the union pass listed jobs and took them
        assert jobs > 0 and rep["bits_jobs"] >= jobs, (tag, rep)
    if route == 1:      # the bit-word kernel's job counter moved
        assert rep["bits_jobs"] > 0, (tag, rep)
    if route == 0 and want["bits"] + want["other"] > 0:
        assert rep["poll_jobs"] > 0, (tag, rep)
    if ucount:
        assert np.array_equal(rep["ucount"], cc.targets(c)), (tag, rep["ucount"], cc.targets(c))
    return route


def _twice(pkg, c, weighted, shared, fn, tag, check):
    """fn(ctx) twice on a fresh context under the forced poll walk, five-launch chain and `shared`;
    after each: check(result), the report, the walk launch's workgroups (one slice row on the first
    poll; one or the hinted rows on the second, whichever lane took it)."""
    x, y, w = cc.points(c.G, weighted)
    nwalk = 8 * -(-c.N // 8)
    rows = max(1, min(cc.POLL_ROWS, -(-int(cc.targets(c).max()) // cc.kPollKPB)))
    with pkg.Context(0) as ctx:
        try:
            ctx.set_points(x, y, w)
            ctx.set_algo("poll")
            ctx.set_chain("five")
            ctx.set_shared(shared)
            ctx.profile(True)
            for rep_no in range(2):
                ctx.profile_read(reset=True)
                out = fn(ctx)
                kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
                slots = _role_slots(pkg, ctx)
                rep = ctx.poll_report(c.N)
                t = (tag, "poll", rep_no)
                check(out, t)
                assert kern.get("disk_index_kernel", 0) == 1 and kern.get("coverage_poll_kernel", 0) == 1, (t, kern)
                assert "fiw_kernel" not in kern and "coverage_tiled_poll_kernel" not in kern, (t, kern)
                # (the pass's kernel is launched whenever a mode but "fp64" is forced)
                assert (kern.get("shared_or_kernel", 0) == 1) == (shared == "bits"), (t, kern)
                wg = slots["coverage_poll_kernel"]
                assert wg in ((nwalk + cc.kSharedWG) * gy for gy in ((1,) if rep_no == 0 else (1, rows))), (t, wg, rows)
                yield rep
        finally:
            ctx.profile_read(reset=True)
            ctx.profile(False)
            ctx.set_shared("auto")
            ctx.set_chain("auto")
            ctx.set_algo("auto")


def _run_case(pkg, orc, name, variant, weighted, shared):
    c, e = _ref(orc, name, variant, weighted)
    tag = (name, variant, "weighted" if weighted else "equal", shared)
    kw = dict(prev=c.prev, d_lim=c.d_lim, tan_half_fov=c.tan_half_fov) if c.cons3 else {}
    want, k = (e.bar, e.k_bar) if c.cons3 else (e.obj, e.k)

    def check_area(got, t):
        bad = np.flatnonzero(got != e.area)
        assert bad.size == 0, (t, "area", bad.size, bad[:8], got[bad[:8]], e.area[bad[:8]])

    def check_poll(got, t):
        bo, bi, objs = got
        bad = np.flatnonzero(objs != want)
        assert bad.size == 0, (t, "objectives", bad.size, bad[:8], objs[bad[:8]], want[bad[:8]])
        assert (bi, bo) == (k, want[k]), (t, "argmin", bi, k, bo, want[k])

    route = None
    for rep in _twice(pkg, c, weighted, shared, lambda ctx: ctx.area_batch(c.C), tag, check_area):
        route = _assert_report(rep, c, weighted, shared, tag)
    # (under cons3 the failed candidates share one inert position: the targets hold for the plain poll)
    for rep in _twice(pkg, c, weighted, shared,
                      lambda ctx: ctx.poll_best(c.C, c.r_max, 1e5, want_all=True, **kw), tag, check_poll):
        _assert_report(rep, c, weighted, shared, tag, ucount=not c.cons3)
    return route


def _want_route(weighted, shared, stands_down=False):
    if shared == "fp64":
        return 0
    return 1 if weighted else (0 if stands_down else 2)


@pytest.mark.parametrize("shared", ["fp64", "bits"])
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("K", cc.K_AXIS)
def test_k_axis(pkg, orc, K, weighted, shared):
    """N = 20 mutually overlapping disks, K on either side of kOrKC (3584), kBitsK = kOrTab (4096) and
    the last K the index deduplicates (6145), and at 7169 (a third candidate chunk of the union pass):
    every disk has min(K, 4335 - i) positions, K under the identity map."""
    route = _run_case(pkg, orc, f"k{K}", "", weighted, shared)
    assert route == _want_route(weighted, shared)


@pytest.mark.parametrize("shared", ["fp64", "bits"])
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
def test_u_axis(pkg, orc, weighted, shared):
    """K = 6145 with 1, 2, 3, 5, 511 .. 513, 2047 .. 2049, 4095 and 4096 positions on consecutive disks
    and 4097 on the large last one: the walk's slices, the bit-word kernel's table groups (a group
    closed by its piece count, a disk split over two groups) and the union pass's table chunks, on
    either side of each."""
    route = _run_case(pkg, orc, "u_axis", "", weighted, shared)
    assert route == _want_route(weighted, shared)


@pytest.mark.parametrize("shared", ["fp64", "bits"])
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("name", ["hub64", "hub65", "hubfirst65", "wide64", "wide65"])
def test_neighbour_and_region_edges(pkg, orc, name, weighted, shared):
    """The two ways the union pass stands down, each from its last fitting shape: a disk with a lower
    neighbour and 64 / 65 upper ones (or_bad 0 / 1; a hub that is disk 0 owns no shared entry and
    never counts), and a disk with a neighbour whose region is 64 / 65 tiles wide (other 0 / 1: the
    wide disk goes to the fp64 jobs under the bit-word kernel too)."""
    route = _run_case(pkg, orc, name, "", weighted, shared)
    assert route == _want_route(weighted, shared, stands_down=name in ("hub65", "wide65"))


@pytest.mark.parametrize("shared", ["fp64", "bits"])
@pytest.mark.parametrize("weighted", [False, True], ids=["equal", "weighted"])
@pytest.mark.parametrize("variant", ["last", "cons3"])
@pytest.mark.parametrize("name", sorted(cc.VARIANTS))
def test_variants(pkg, orc, name, variant, weighted, shared):
    """One case per family with the last candidate as the strict minimiser (a dropped last candidate
    shows in the argmin as well as in its own objective) and with a cons3 limit that fails some rows
    and keeps others."""
    _run_case(pkg, orc, name, variant, weighted, shared)


def test_auto_hint_reaches_the_union_pass(pkg, orc):
    """set_shared("auto"), K = kOrKC + 1 on equal weights: the union pass is launched on a hint (the
    lane's earlier polls' count of disks with neighbours) and the context's lanes take turns, so a run
    of twelve polls: every result is the oracle's, shared_or_kernel is in the profile, and the last
    poll's report shows the union pass's route with jobs taken."""
    c, e = _ref(orc, f"k{cc.kOrKC + 1}")
    x, y, w = cc.points(c.G, False)
    with pkg.Context(0) as ctx:
        try:
            ctx.set_points(x, y, w)
            ctx.set_algo("poll")
            ctx.set_chain("five")
            ctx.set_shared("auto")
            ctx.profile(True)
            ctx.profile_read(reset=True)
            outs, reps = [], []
            for _ in range(12):
                outs.append(ctx.area_batch(c.C))
                reps.append(ctx.poll_report(c.N))
            kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        finally:
            ctx.profile_read(reset=True)
            ctx.profile(False)
            ctx.set_shared("auto")
            ctx.set_chain("auto")
            ctx.set_algo("auto")
    for q, g in enumerate(outs):
        bad = np.flatnonzero(g != e.area)
        assert bad.size == 0, (q, bad.size, bad[:8], g[bad[:8]], e.area[bad[:8]])
    assert kern.get("shared_or_kernel", 0) > 0, kern
    # bits_on = 1 wherever the pass was launched: 19 disks with neighbours > kBitsMinDisks
    assert all(cc.shared_route(r, 1, 1) == 2 and np.array_equal(r["ucount"], cc.targets(c)) for r in reps), reps
    took = [r for r in reps if sum(r[f"or_jobs{b}"] for b in range(4)) > 0]
    assert took and all(r["bits_jobs"] > 0 for r in took), reps


def test_positions_past_two_to_the_16_through_the_bit_word_kernel(pkg, orc):
    """K = 65,600 under the identity map, three mutually overlapping disks, the weighted list, the
    bit-word kernel forced: the last chunk's 64 candidates sit at positions 65,536 .. 65,599. Every
    job here fits the kernel's map-value cache by size ((1 + neighbours) x candidates <= kBitsUC),
    but the cache holds 16 bits a value; a position cut to 16 bits lies inside the first table group
    and takes candidate k - 65,536's word (a wrong sum, nothing out of range). The kernel takes the
    cache only when every disk of the job has at most 2^16 positions."""
    c, e = _ref(orc, "u16", weighted=True)
    x, y, w = cc.points(c.G, True)
    with pkg.Context(0) as ctx:
        try:
            ctx.set_points(x, y, w)
            ctx.set_algo("poll")
            ctx.set_chain("five")
            ctx.set_shared("bits")
            got = ctx.area_batch(c.C)
            rep = ctx.poll_report(c.N)
        finally:
            ctx.set_shared("auto")
            ctx.set_chain("auto")
            ctx.set_algo("auto")
    assert cc.shared_route(rep, 2, 0) == 1 and rep["bits"] == 2 and rep["bits_jobs"] > 0, rep
    assert np.array_equal(rep["ucount"], np.full(c.N, c.K)), rep
    bad = np.flatnonzero(got != e.area)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], e.area[bad[:8]])
