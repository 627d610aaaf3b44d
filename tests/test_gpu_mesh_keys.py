"""Keys in mesh units (MAC_OPT_MESH_KEYS = MAC_KEYS_MESH; csrc/mesh_key.h) through every place a key is
written or read on the device: both prep launches, the disk index, fiw_kernel and fin2_kernel.

Reference side: test_gpu_granularity.py's (TDM_STATIC_opt.mads over the C oracle with host callables,
one trial point at a time; libmaxcover is not on that side), shared with that file by import, so a
whole-suite run computes each reference once. Every comparison is exact. Beside the results, the tests
assert where the decision was taken: the fused chain's hint reports (no disk on one position per
candidate), the launches AUTO made, and the index's position counts against the distinct disks of the
mirror's own basis. The N ~ 512 cases compare the build with itself (mesh keys on one context, value
keys on another); the value-key path is the one pinned against the oracle."""
import math

import numpy as np
import pytest

import test_gpu_granularity as tg
import test_gpu_prog as tp
from test_gpu_poll_vars import FOV, TAN50, _chain, _recipe

pytestmark = pytest.mark.gpu

MADS = tg.MADS
GRANS = tg.GRANS
_TIMES = tg._TIMES


@pytest.fixture
def mk(ctx):
    """The session's context with mesh keys on for one test."""
    ctx.set_mesh_keys(True)
    try:
        yield ctx
    finally:
        ctx.set_mesh_keys(False)


# ---------------------------------------------------------------- the option on a live context

def test_option_values(pkg, ctx):
    """0 and 1 are accepted before and after points are set, 2 (and -1) refused, the mode kept."""
    lib = pkg._lib
    with pkg.Context(0) as c2:
        for when in ("before", "after"):
            if when == "after":
                c2.set_points_records(_recipe(pkg, 3, 7, 320, 40)[0])
            for v in (1, 0, 1, 0):
                c2.set_option(lib.MAC_OPT_MESH_KEYS, v)
            for v in (2, -1, 7):
                with pytest.raises(Exception):
                    c2.set_option(lib.MAC_OPT_MESH_KEYS, v)


# ---------------------------------------------------------------- 1. whole runs against the oracle loop

@pytest.mark.parametrize("chain", ["auto", "five", "fused"])
@pytest.mark.parametrize("driver", ["run", "stepper"])
@pytest.mark.parametrize("gran", GRANS)
def test_a_chain_case(mk, pkg, orc, gran, driver, chain):
    """N = 12 (K = 72: the column-triple prep), every granularity of test_gpu_granularity's, mads_run and
    the stepper, each chain: the oracle loop's iterates, and no disk of a fused poll off the packed keys."""
    rec, x0, r_max, ref = tg._chain_reference(pkg, orc, gran)
    if chain == "auto":   # (a context of its own: AUTO reads the context's routing history)
        with pkg.Context(0) as c2:
            c2.set_mesh_keys(True)
            _chain_case(c2, pkg, rec, x0, r_max, ref, gran, driver, chain)
    else:
        _chain_case(mk, pkg, rec, x0, r_max, ref, gran, driver, chain)


def _chain_case(ctx, pkg, rec, x0, r_max, ref, gran, driver, chain):
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: tg._stepper_run(ctx, a[0], a[1], **k))
    ctx.profile_fused(reset=True)
    got, kern = tg._profiled(ctx, chain, lambda: (run(x0, r_max, 1e5, granularity=gran, **tg._c3kw(ref),
                                                      **tg._native(MADS)), ctx.profile_fused(reset=True)))
    got, fused = got
    print(gran, driver, chain, kern, fused, {k: v for k, v in got[1].items() if k not in _TIMES})
    tg._check(got, ref)
    assert kern.get("prep_kernel", 0) >= ref["it"] - got[1]["rejected_polls"], kern
    if chain == "fused":
        assert kern.get("fiw_kernel", 0) > 0, kern
        if driver == "stepper":   # (the stepper's lane reads the hints back poll by poll)
            assert fused["reports"] > 0, fused
        assert fused["ident_sum"] == 0, fused   # every key packed: (1, 0.1) and (0.1, 0.1) too
    if chain == "five":
        assert kern.get("coverage_poll_kernel", 0) > 0 and "fiw_kernel" not in kern, kern
        # every poll took the poll walk (the per-candidate walk's one launch is f(x0), K = 1)
        assert kern["coverage_poll_kernel"] == kern["disk_index_kernel"], kern
        assert kern.get("coverage_tiled_poll_kernel", 0) <= 1, kern
    if chain == "auto":
        # this recipe is uncrowded: AUTO follows the crowding estimate alone, fractional g or not
        assert kern.get("fiw_kernel", 0) > 0, kern


def test_a_part_full_prep_workgroups(mk, pkg, orc):
    """N = 13 (K = 78), (1, 0.1): mads_run and the stepper under each chain."""
    ctx = mk
    gran = (1.0, 0.1)
    rec, x0, r_max = _recipe(pkg, 13, 2024, 320, 160)
    ref = tg._reference(pkg, orc, ("chain", 13, gran), rec, x0, r_max, gran)
    assert ref["polled"] == 30 * 78 and ref["f"] < ref["f0"] and ref["succ"] >= 3
    ctx.set_points_records(rec)
    for chain in ("five", "fused"):
        for run in (ctx.mads_run, lambda *a, **k: tg._stepper_run(ctx, a[0], a[1], **k)):
            got, kern = tg._profiled(ctx, chain, lambda: run(x0, r_max, 1e5, granularity=gran, **tg._c3kw(ref),
                                                             **tg._native(MADS)))
            tg._check(got, ref)
            assert ("fiw_kernel" in kern) == (chain == "fused"), (chain, kern)


# ---------------------------------------------------------------- 2. one poll against the oracle

def _one_poll(ctx, pkg, orc, rec, x0, r_max, gran, ell, chain, prev=None, seed=99, poll_vars="xyr"):
    """One stepper poll at mesh index ell against the host-built candidate matrix, column by column
    through orc.ref_objective and cons3: (bo, bi) equal, and under the five-launch chain every disk's
    position count equal to its distinct feasible triples (+ 1 inert when a candidate failed).
    Returns (ucount or None, the distinct-disk counts, K, basis, feasible mask)."""
    TS, TC, wl = pkg.TDM_STATIC_opt, pkg.TDM_Constraints, pkg.workloads
    N = x0.size // 3
    n_p = TS.polled_count(x0.size, poll_vars)
    g = pkg._lib.mesh_granularity(gran, x0.size)
    c3 = TC.create_cons3(x0 if prev is None else prev, FOV, np.full(N, 10.0))
    B = wl.ltmads_basis(n_p, ell, wl.SplitMix64(seed))
    X = TS.poll_matrix(x0, TS.scaled_basis(B.astype(np.float64), g))
    feas = np.array([bool(c3(v)) for v in X])
    obj = np.array([orc.ref_objective(v, rec, r_max, 1e5) if ok else math.inf for v, ok in zip(X, feas)])
    want_i = int(np.argmin(obj)) if feas.any() else -1
    want_o = float(obj[want_i]) if feas.any() else math.inf
    ctx.set_points_records(rec)
    _chain(ctx, chain)
    st = ctx.mads_stepper(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, n_iter=1,
                          ell0=ell, ell_max=ell, seed=seed, granularity=gran, poll_vars=poll_vars)
    try:
        done, bo, bi = st.poll()
        assert not done
        uc = ctx.poll_report(N)["ucount"] if chain == "five" else None
    finally:
        st.close()
        _chain(ctx, "auto")
    assert (bo, bi) == (want_o, want_i), (bo, bi, want_o, want_i)
    want = np.array([len({X[k, [i, N + i, 2 * N + i]].tobytes() for k in np.flatnonzero(feas)}) +
                     (0 if feas.all() else 1) for i in range(N)])
    return uc, want, X.shape[0], B, feas


@pytest.mark.parametrize("chain", ["five", "fused"])
@pytest.mark.parametrize("case", ["real", "negzero", "two53", "dead_radii"])
def test_b_one_poll(mk, pkg, orc, case, chain):
    """N = 12, one poll: a real-valued incumbent (x0 + 0.3); an incumbent holding -0.0 and one holding
    2^53 (absorption: a second position at most); radii 0.25 with g_r = 0.125 at ell = 2, so that some
    candidates have r = 0 and r < 0. Under the five-launch chain every disk deduplicates (ucount < K) but
    the two that hold -0.0."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    N, gran, ell = 12, (1.0, 0.1), 2
    prev = None
    if case == "real":
        x0 = x0 + 0.3
    elif case == "negzero":
        x0 = x0.copy()
        x0[0], x0[N + 1] = -0.0, -0.0
    elif case == "two53":
        x0 = x0.copy()
        x0[2] = 2.0 ** 53
    else:
        x0 = x0.copy()
        x0[2 * N:] = 0.25
        gran = (1.0, 0.125)
    uc, want, K, B, feas = _one_poll(mk, pkg, orc, rec, x0, r_max, gran, ell, chain, prev)
    assert feas.sum() > K // 2
    if case == "dead_radii":
        g = pkg._lib.mesh_granularity(gran, x0.size)
        r = x0[2 * N:, None] + np.concatenate([B, -B], axis=1)[2 * N:] * g[2 * N:, None]
        assert np.any(r == 0.0) and np.any(r < 0.0)
    if uc is not None:
        print(case, uc, want)
        if case == "negzero":
            # The minus candidate of a zero draw on a -0.0 incumbent is -0.0 - 0.0 = -0.0, and its decode
            # -0.0 + g * 0 is +0.0: the check refuses the word and those two disks take the identity map.
            assert np.all(uc[:2] == K) and np.array_equal(uc[2:], want[2:]) and np.all(uc[2:] < K), (uc, want)
            return
        assert np.all(uc < K), uc
        if case == "two53":   # (odd draws are absorbed at 2^53: two words, one double, a second position)
            assert np.array_equal(np.delete(uc, 2), np.delete(want, 2)) and want[2] <= uc[2]
        else:
            assert np.array_equal(uc, want), (uc, want)


@pytest.mark.parametrize("ell", [9, 10])
def test_b_past_the_field(mk, pkg, orc, ell):
    """ell0 = ell_max = 9 and 10 with g = 0.005 everywhere: cons3 passes (steps of at most 5.12), the
    radius's diagonal draw +-512 (and at ell = 10 every diagonal, +-1024) does not pack, and the disk
    takes the identity map: ucount = K. The fused chain gives the same poll result."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    uc, _, K, B, feas = _one_poll(mk, pkg, orc, rec, x0, r_max, 0.005, ell, "five")
    assert feas.all() and np.abs(B).max() == 1 << ell
    assert np.all(uc == K), uc
    _one_poll(mk, pkg, orc, rec, x0, r_max, 0.005, ell, "fused")


def test_b_value_keys_take_the_identity_map_here(ctx, pkg, orc):
    """The same (1, 0.1) poll with value keys: every disk on one position per candidate (what mesh keys
    remove), the result unchanged."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    uc, _, K, _, _ = _one_poll(ctx, pkg, orc, rec, x0, r_max, (1.0, 0.1), 2, "five")
    assert np.all(uc == K), uc


# ---------------------------------------------------------------- 3. xy-only polls

@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_c_xy_poll(mk, pkg, orc, driver):
    """N = 12, (0.5, 0.125), poll_vars="xy" (K = 48: below the poll chain): test_gpu_granularity's case
    with mesh keys on; the radii bytes unchanged."""
    tg.test_c_xy_poll(mk, pkg, orc, driver)


@pytest.mark.parametrize("chain", ["five", "fused"])
def test_c_xy_poll_in_the_chain(mk, pkg, orc, chain):
    """N = 18, xy-only (K = 72, n_p = 36: the poll chain through prep_kernel's pair layout, the radii
    held with m = 0), (0.5, 0.125), against the oracle loop."""
    ctx = mk
    gran = (0.5, 0.125)
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    ref = tg._reference(pkg, orc, ("xy18", gran), rec, x0, r_max, gran, poll_vars="xy")
    assert ref["polled"] == 30 * 72 and ref["f"] < ref["f0"] and ref["succ"] > 3
    ctx.set_points_records(rec)
    for run in (ctx.mads_run, lambda *a, **k: tg._stepper_run(ctx, a[0], a[1], **k)):
        got, kern = tg._profiled(ctx, chain, lambda: run(x0, r_max, 1e5, granularity=gran, poll_vars="xy",
                                                         **tg._c3kw(ref), **tg._native(MADS)))
        tg._check(got, ref)
        assert got[0][36:].tobytes() == x0[36:].tobytes()
        assert ("fiw_kernel" in kern) == (chain == "fused"), kern
    uc, want, K, _, _ = _one_poll(ctx, pkg, orc, rec, x0, r_max, gran, 2, "five", poll_vars="xy")
    assert np.all(uc < K) and np.array_equal(uc, want), (uc, want)


# ---------------------------------------------------------------- 4. one constraint of each kind

@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_d_swarm_constraint(mk, pkg, orc, driver):
    tg.test_e_swarm_constraint(mk, pkg, orc, driver)


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_d_motion_constraints(mk, pkg, orc, driver):
    tg.test_e_motion_constraints(mk, pkg, orc, driver)


@pytest.mark.parametrize("mode", ["auto", "five", "fused"])
@pytest.mark.parametrize("N", [5, 12])
def test_d_progressive_barrier(mk, pkg, orc, N, mode):
    """create_cons1_progressive with penalty 0 on (1, 0.125): each polled centre is its own key base.
    N = 5 (K = 30: the loop below the chains) and N = 12 (K = 72: the chains)."""
    res, st, kern = tp._run(mk, pkg, orc, mode, N, 36.0, gran=(1.0, 0.125), profile=True)
    assert res.status.dominating >= 1
    if N == 5:
        assert res.status.two_centre_polls >= 1
    if N == 12 and mode == "fused":   # (AUTO on the session's context follows its routing history)
        assert kern.get("fiw_kernel", 0) > 0, kern


# ---------------------------------------------------------------- 5. shards and speculation

def test_e_two_shards(mk, pkg, orc):
    """Two shard steppers over one poll (k0 != 0: prep_kernel's plain layout), (0.5, 0.125)."""
    tg.test_f_two_shards(mk, pkg, orc)


def test_e_speculation(mk, pkg, orc):
    tg.test_f_speculation(mk, pkg, orc)


@pytest.mark.parametrize("chain", ["five", "fused"])
def test_e_two_shards_at_1_01(mk, pkg, orc, chain):
    """Two shard steppers at (1, 0.1), each chain forced."""
    from importlib import import_module
    d = import_module(pkg.__name__ + ".dist")
    ctx = mk
    gran = (1.0, 0.1)
    rec, x0, r_max, ref = tg._chain_reference(pkg, orc, gran)
    kw = dict(granularity=gran, **tg._c3kw(ref), **tg._native(MADS))
    ctx.set_points_records(rec)
    K = 72
    _chain(ctx, chain)
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=sh, **kw) for sh in ((0, K // 2), (K // 2, K))]
    try:
        while True:
            res = [s_.poll() for s_ in steppers]
            if res[0][0]:
                break
            bo, bi = d.reduce_best([r[1] for r in res], [r[2] for r in res])
            for s_ in steppers:
                s_.update(bo, bi)
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, ref["x"]) and st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["successes"] == ref["succ"] and st["slot_fallbacks"] == 0
    finally:
        for s_ in steppers:
            s_.close()
        _chain(ctx, "auto")


# ---------------------------------------------------------------- 6. the block edges (the build against itself)

@pytest.mark.parametrize("chain", ["five", "fused"])
@pytest.mark.parametrize("N", [511, 512, 513])
def test_f_block_edges_against_value_keys(pkg, N, chain):
    """N = 511, 512, 513 (K = 6N: one block of UAVs full, and one past it: prep_kernel's second block),
    (1, 0.125), 6 iterations: mesh keys on one context against value keys on a second. THE BUILD AGAINST
    ITSELF, not the oracle (a loop at K = 3072 takes minutes): iterates, f, counts and statistics equal."""
    rec, x0, r_max = _recipe(pkg, N, 2024, 100, 600, radii=12.0)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50, n_iter=6, ell0=2, ell_max=5, seed=99,
              granularity=(1.0, 0.125))
    out = []
    for keys in (False, True):
        with pkg.Context(0) as c2:
            c2.set_points_records(rec)
            c2.set_mesh_keys(keys)
            _chain(c2, chain)
            xs, st = c2.mads_run(x0, r_max, 1e5, **kw)
            out.append((xs, {k: v for k, v in st.items() if k not in _TIMES}))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1] == out[1][1]
    assert out[0][1]["iterations"] == 6 and out[0][1]["evaluations"] == 1 + 6 * 6 * N
    assert out[0][1]["successes"] >= 1 and out[0][1]["feasible_evaluations"] > 0


# ---------------------------------------------------------------- 7. off is off

def test_g_off_is_off(pkg):
    """Option 1 with no mesh, and option 0 with a mesh, give the launches (roles and counts), outputs and
    statistics of a context that never touched the option."""
    N = 12
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50, n_iter=30, ell0=2, ell_max=5, seed=99)

    def run(opt, **extra):
        with pkg.Context(0) as c2:
            if opt is not None:
                c2.set_option(pkg._lib.MAC_OPT_MESH_KEYS, opt)
            c2.set_points_records(rec)
            c2.profile(True)
            c2.profile_read(reset=True)
            xs, st = c2.mads_run(x0, r_max, 1e5, **kw, **extra)
            kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
            a = tg._stepper_run(c2, x0, r_max, **kw, **extra)
        strip = lambda s: {k: v for k, v in s.items() if k not in _TIMES}   # noqa: E731
        return xs.tobytes(), strip(st), kern, a[0].tobytes(), strip(a[1])

    base = run(None)
    assert base[1]["iterations"] > 3
    assert run(1) == base                                  # no mesh
    assert run(1, granularity=np.ones(3 * N)) == base      # the unit mesh is no mesh
    meshed = run(None, granularity=(1.0, 0.125))
    assert run(0, granularity=(1.0, 0.125)) == meshed      # value keys named explicitly
    assert meshed[0] != base[0]
