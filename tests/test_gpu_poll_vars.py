"""The native MADS driver's xy-only poll (MAC_POLL_XY: mac_mads_run_opts / mac_mads_begin_opts,
include/maxcover.h; the reference's CustomPoll, src/TDM_STATIC_opt.jl:15-44): the basis drawn over
the n_p = 2N variables x, y, 4N candidates per poll, the radii held bit for bit.

Reference side: the Python driver TDM_STATIC_opt.mads(poll_vars="xy") with a plain callable objective
over the C oracle (orc.ref_objective, one trial point at a time) and cons1 / cons3 (and cons8) as
host callables, the recipe of test_gpu_parity.test_native_mads_matches_oracle_loop; libmaxcover is
not on that side (pinned on the CPU by test_poll_vars_host.py). Every comparison is exact. Each
reference run is computed once and shared by the modes compared with it."""
import ctypes
import math
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)
MADS = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
NATIVE = dict(n_iter=30, ell0=2, ell_max=5, seed=99)
_TIMES = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")
_REF = {}


def _grid(pkg, G=160):
    x, y, w = pkg.workloads.grid_points(G)
    return np.stack([x, y, w, w, np.zeros_like(x)], axis=1)


def _recipe(pkg, N, seed, lo, span, radii=36.0):
    rng = pkg.workloads.SplitMix64(seed)
    x0 = np.concatenate([np.round(lo + rng.uniform(N) * span), np.round(lo + rng.uniform(N) * span),
                         np.full(N, radii)])
    return _grid(pkg), x0, np.full(N, 30.0 * TAN50)


def _reference(pkg, orc, key, rec, x0, r_max, swarm=(), mads_kw=MADS, poll_vars="xy"):
    if key not in _REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        N = x0.size // 3
        c3 = TC.create_cons3(x0, FOV, np.full(N, 10.0))

        def oracle_objective(v):
            return orc.ref_objective(v, rec, r_max, 1e5)

        res = TS.mads(x0, oracle_objective, [TC.cons1, *swarm, c3], poll_vars=poll_vars, **mads_kw)
        _REF[key] = dict(x=res.x if res.x is not None else res.i, f=res.x_cost if res.x is not None else math.inf,
                         it=res.status.iteration, limit=res.status.optimization_status == "MeshPrecisionLimit",
                         evals=res.status.function_evaluations, succ=res.status.successes,
                         polled=res.status.iteration * 2 * TS.polled_count(x0.size, poll_vars), c3=c3,
                         f0=oracle_objective(x0))
    return _REF[key]


def _check(got, ref, x0):
    xn, st = got
    N = x0.size // 3
    assert np.array_equal(xn, ref["x"])
    assert xn[2 * N:].tobytes() == x0[2 * N:].tobytes()   # the radii: x0's doubles
    assert st["f"] == ref["f"]
    assert st["iterations"] == ref["it"]
    assert (st["status"] == 0) == ref["limit"]
    assert st["evaluations"] == 1 + ref["polled"]
    assert st["feasible_evaluations"] == ref["evals"] - 1
    assert st["successes"] == ref["succ"]
    assert st["slot_fallbacks"] == 0


def _c3kw(ref):
    c3 = ref["c3"]
    return dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov)


def _stepper_run(ctx, x0, r_max, **kw):
    st = ctx.mads_stepper(x0, r_max, 1e5, **kw)
    try:
        assert st.candidates == 4 * (x0.size // 3) and st.shard == (0, st.candidates)
        while True:
            done, bo, bi = st.poll()
            if done:
                break
            assert -1 <= bi < st.candidates
            st.update(bo, bi)
        return st.result()
    finally:
        st.close()


def _chain(ctx, chain):
    ctx.set_algo("auto")
    ctx.set_chain(chain)


@pytest.mark.parametrize("chain", ["auto", "five", "fused"])
@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_a_pair_prep(ctx, pkg, orc, driver, chain):
    """N = 18 with cons3: K = 72 runs the poll chain, n_p = 36 takes the pair prep; mads_run (the
    pipelined loop) and the stepper, each chain."""
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    ref = _reference(pkg, orc, "a18", rec, x0, r_max)
    assert ref["polled"] == 30 * 72 and ref["f"] < ref["f0"] and ref["succ"] > 3
    ctx.set_points_records(rec)
    _chain(ctx, chain)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
        got = run(x0, r_max, 1e5, poll_vars="xy", **_c3kw(ref), **NATIVE)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        _chain(ctx, "auto")
    _check(got, ref, x0)
    assert kern.get("prep_kernel", 0) >= ref["it"] - got[1]["rejected_polls"], kern   # the poll chain ran
    if chain == "fused":
        assert kern.get("fiw_kernel", 0) > 0, kern
    if chain == "five":
        assert kern.get("coverage_poll_kernel", 0) > 0 and "fiw_kernel" not in kern, kern


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_b_non_pair_prep(ctx, pkg, orc, driver):
    """N = 17: n_p = 34 is no multiple of 4 (the non-pair prep), K = 68."""
    rec, x0, r_max = _recipe(pkg, 17, 2024, 320, 160)
    ref = _reference(pkg, orc, "b17", rec, x0, r_max)
    assert ref["polled"] == 30 * 68 and ref["f"] < ref["f0"]
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    _check(run(x0, r_max, 1e5, poll_vars="xy", **_c3kw(ref), **NATIVE), ref, x0)


@pytest.mark.parametrize("N,seed,lo,span", [(5, 7, 320, 40), (2, 39, 390, 20), (1, 39, 400, 1)])
def test_c_below_the_poll_chain(ctx, pkg, orc, N, seed, lo, span):
    """K = 20, 8, 4: the per-candidate walk and the stepper loop."""
    rec, x0, r_max = _recipe(pkg, N, seed, lo, span)
    ref = _reference(pkg, orc, f"c{N}", rec, x0, r_max)
    assert ref["f"] < ref["f0"] and ref["polled"] == ref["it"] * 4 * N
    ctx.set_points_records(rec)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        got = ctx.mads_run(x0, r_max, 1e5, poll_vars="xy", **_c3kw(ref), **NATIVE)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    _check(got, ref, x0)
    assert "prep_kernel" not in kern   # (no poll chain at this size)
    _check(_stepper_run(ctx, x0, r_max, poll_vars="xy", **_c3kw(ref), **NATIVE), ref, x0)


def test_d_two_prep_blocks_against_the_host_mirror(ctx, pkg):
    """N = 600 (two UAV blocks in the prep, n_p = 1200, K = 2400): the native stepper against
    TDM_STATIC_opt.PollStepper(poll_vars="xy") whose polls are the matrix poll (Context.poll_best) —
    the build against itself: size coverage, as test_e_larger_n_stepper_against_the_host_mirror."""
    TS = pkg.TDM_STATIC_opt
    N = 600
    rng = pkg.workloads.SplitMix64(1600)
    side = 25
    ix, iy = np.divmod(np.arange(N), side)
    x0 = np.concatenate([100.0 + 18.0 * ix + np.round(rng.uniform(N) * 2.0 - 1.0),
                         100.0 + 18.0 * iy + np.round(rng.uniform(N) * 2.0 - 1.0), np.full(N, 12.25)])
    x, y, w = pkg.workloads.grid_points(70)
    ctx.set_points(x, y, w)
    r_max = np.full(N, 12.25)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50)
    f0, i0 = ctx.poll_best(x0[None, :], r_max, 1e5, **kw)
    assert i0 == 0 and math.isfinite(f0)
    shapes = []

    def poll_fn(Xs):
        shapes.append(Xs.shape)
        return ctx.poll_best(Xs, r_max, 1e5, **kw)

    mirror = TS.PollStepper(x0, f0, poll_fn, N_iter=3, ell0=1, ell_max=2, seed=77, poll_vars="xy")
    st = ctx.mads_stepper(x0, r_max, 1e5, n_iter=3, ell0=1, ell_max=2, seed=77, poll_vars="xy", **kw)
    try:
        assert st.n_polled == 1200 and st.candidates == 2400
        polls = 0
        while True:
            want = mirror.poll()
            got = st.poll()
            assert got[0] == want[0]
            if got[0]:
                break
            polls += 1
            assert (got[1], got[2]) == (want[1], want[2]), (polls, got, want)
            mirror.update(want[1], want[2])
            st.update(got[1], got[2])
        xs, stats = st.result()
    finally:
        st.close()
    xm, sm = mirror.result()
    assert polls == 3 and shapes == [(2400, 1800)] * 3
    assert np.array_equal(xs, xm) and stats["f"] == sm["f"] and stats["evaluations"] == sm["evaluations"] == 7201
    assert xs[2 * N:].tobytes() == x0[2 * N:].tobytes()


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_e_non_integer_radii(ctx, pkg, orc, driver):
    """Radii exactly at r_max = 30 tan 50 deg (no integer): x_out's radii are x0's doubles, the
    penalty term is exactly 0 (f = -area), and the area gain is the oracle's."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160, radii=30.0 * TAN50)
    assert x0[-1] != round(x0[-1]) and np.array_equal(x0[24:], r_max)
    ref = _reference(pkg, orc, "e12", rec, x0, r_max)
    P = orc.PointerList(rec)
    a0, a1 = P.area_batch(x0[None, :])[0], P.area_batch(ref["x"][None, :])[0]
    assert ref["f0"] == -a0 and ref["f"] == -a1 and a1 > a0   # (the penalty is exactly 0 on that side)
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, poll_vars="xy", **_c3kw(ref), **NATIVE)
    _check(got, ref, x0)
    assert got[1]["f"] == -ctx.area(got[0])
    assert ref["f0"] - got[1]["f"] == a1 - a0


@pytest.mark.parametrize("driver", ["run", "stepper"])
@pytest.mark.parametrize("d_sep", [4.0, 8.0])
def test_f_swarm_mask_over_xy_candidates(ctx, pkg, orc, d_sep, driver):
    """N = 18 under cons8 (x0's closest pair is sqrt(17) apart: a feasible start under 4, an
    infeasible one that recovers under 8), against the oracle loop with create_cons8 as a host
    callable."""
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    rejected = [0]
    c8 = pkg.TDM_Constraints.create_cons8(d_sep)

    def counted(v):
        ok = bool(c8(v))
        rejected[0] += not ok
        return ok

    fresh = ("f18", d_sep) not in _REF
    ref = _reference(pkg, orc, ("f18", d_sep), rec, x0, r_max, swarm=[counted])
    if fresh:
        ref["rejected"] = rejected[0]
    free = _reference(pkg, orc, "a18", rec, x0, r_max)
    assert 0 < ref["rejected"] < ref["polled"] and math.isfinite(ref["f"])
    assert ref["evals"] < free["evals"]
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, poll_vars="xy", cons={"d_sep": d_sep}, **_c3kw(ref), **NATIVE)
    _check(got, ref, x0)


@pytest.mark.parametrize("world", [2, 3])
def test_g_sharded_steppers(ctx, pkg, orc, world):
    """`world` steppers over the shards of [0, 4N) in one process: every one ends on mads_run's
    result, and the shards' feasible evaluations add up to the run's."""
    d = import_module(pkg.__name__ + ".dist")
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    ref = _reference(pkg, orc, "a18", rec, x0, r_max)
    kw = dict(poll_vars="xy", **_c3kw(ref), **NATIVE)
    ctx.set_points_records(rec)
    want_x, want = ctx.mads_run(x0, r_max, 1e5, **kw)
    _check((want_x, want), ref, x0)
    K = 4 * 18
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=d.shard_range(K, r, world), **kw) for r in range(world)]
    try:
        polls = 0
        while True:
            res = [s_.poll() for s_ in steppers]
            assert len({r[0] for r in res}) == 1
            if res[0][0]:
                break
            polls += 1
            for (lo, hi), r in zip((s_.shard for s_ in steppers), res):
                assert r[2] == -1 or lo <= r[2] < hi
            bo, bi = d.reduce_best([r[1] for r in res], [r[2] for r in res])
            for s_ in steppers:
                s_.update(bo, bi)
        assert polls == want["iterations"]
        feas = 0
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, want_x)
            assert {k: st[k] for k in ("f", "iterations", "evaluations", "successes")} == \
                   {k: want[k] for k in ("f", "iterations", "evaluations", "successes")}
            assert st["slot_fallbacks"] == 0
            feas += st["feasible_evaluations"]
        assert feas == want["feasible_evaluations"]
    finally:
        for s_ in steppers:
            s_.close()


@pytest.mark.parametrize("world", [2, 3])
def test_g_speculative_steppers(ctx, pkg, orc, world):
    """The speculative loop (mac_mads_poll_ahead / mac_mads_advance) on xy steppers."""
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    ref = _reference(pkg, orc, "a18", rec, x0, r_max)
    kw = dict(poll_vars="xy", **_c3kw(ref), **NATIVE)
    ctx.set_points_records(rec)
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, **kw) for _ in range(world)]
    try:
        useful = 0
        while True:
            res = [s_.poll_ahead(j) for j, s_ in enumerate(steppers)]
            finished = False
            for j in range(world):
                done, bo, bi, fe = res[j]
                if done:
                    finished = True
                    break
                useful += fe
                moved = [s_.advance(bo, bi) for s_ in steppers]
                assert len(set(moved)) == 1
                if moved[0]:
                    break
            if finished:
                break
        assert useful == ref["evals"] - 1
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, ref["x"]) and xs[36:].tobytes() == x0[36:].tobytes()
            assert st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["successes"] == ref["succ"]
            assert st["slot_fallbacks"] == 0
    finally:
        for s_ in steppers:
            s_.close()


def test_g_dist_loops_on_an_xy_stepper(ctx, pkg, orc):
    """dist.mads_loop and dist.mads_loop_speculative (one rank) drive an xy stepper unchanged."""
    d = import_module(pkg.__name__ + ".dist")
    rec, x0, r_max = _recipe(pkg, 18, 2024, 320, 160)
    ref = _reference(pkg, orc, "a18", rec, x0, r_max)
    ctx.set_points_records(rec)
    for loop in (d.mads_loop, d.mads_loop_speculative):
        st = ctx.mads_stepper(x0, r_max, 1e5, poll_vars="xy", **_c3kw(ref), **NATIVE)
        try:
            _check(loop(st), ref, x0)
        finally:
            st.close()


@pytest.mark.parametrize("N", [12, 5])
def test_h_off_is_off(pkg, N):
    """opts = NULL and MAC_POLL_XYR through mac_mads_run_opts (with and without a cons) give
    mac_mads_run's outputs, statistics and launch counts, in the pipelined loop (N = 12) and the
    stepper loop (N = 5)."""
    lib = pkg._lib
    L = pkg.load_library()
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    d_lim = np.full(N, 10.0)
    dp = ctypes.POINTER(ctypes.c_double)
    off = lib.Cons(math.nan, math.nan, math.nan)

    def plain(c2):
        return c2.mads_run(x0, r_max, 1e5, prev=x0, d_lim=d_lim, tan_half_fov=TAN50, **NATIVE)

    def through_opts(opts, cons):
        def run(c2):
            out = np.empty_like(x0)
            prm = lib.MadsParams(30, 2, 5, 99)
            st = lib.MadsStats()
            rc = L.mac_mads_run_opts(c2._h, x0.ctypes.data_as(dp), x0.size, r_max.ctypes.data_as(dp), 1e5,
                                     x0.ctypes.data_as(dp), d_lim.ctypes.data_as(dp), TAN50, ctypes.byref(prm),
                                     out.ctypes.data_as(dp), ctypes.byref(st),
                                     ctypes.byref(cons) if cons is not None else None,
                                     ctypes.byref(opts) if opts is not None else None)
            assert rc == lib.MAC_OK, L.mac_last_error()
            return out, {k: getattr(st, k) for k, _ in lib.MadsStats._fields_}
        return run

    runs = []
    for run in (plain, through_opts(None, None), through_opts(lib.MadsOpts(lib.MAC_POLL_XYR), None),
                through_opts(lib.MadsOpts(lib.MAC_POLL_XYR), off), through_opts(None, off)):
        with pkg.Context(0) as c2:   # (fresh contexts: the same routing history)
            c2.set_points_records(rec)
            c2.profile(True)
            c2.profile_read(reset=True)
            xs, st = run(c2)
            kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
        runs.append((xs, {k: v for k, v in st.items() if k not in _TIMES}, kern))
    for xs, st, kern in runs[1:]:
        assert np.array_equal(xs, runs[0][0])
        assert st == runs[0][1]
        assert kern == runs[0][2]
    assert runs[0][1]["iterations"] > 3 and runs[0][1]["evaluations"] == 1 + 6 * N * runs[0][1]["iterations"]
    # the keyword's default and "xyr" are the plain call too; the stepper's shard stays (0, 6N)
    with pkg.Context(0) as c2:
        c2.set_points_records(rec)
        xs, st = c2.mads_run(x0, r_max, 1e5, prev=x0, d_lim=d_lim, tan_half_fov=TAN50, poll_vars="xyr", **NATIVE)
        assert np.array_equal(xs, runs[0][0]) and st["f"] == runs[0][1]["f"]
        s_ = c2.mads_stepper(x0, r_max, 1e5, poll_vars="xyr", **NATIVE)
        assert s_.shard == (0, 6 * N) and s_.candidates == 6 * N and s_.n_polled == 3 * N
        s_.close()


def test_i_shard_limits(ctx, pkg):
    """An xy stepper's shards lie in [0, 4N]: the full poll's (0, 2 * 3N) is MAC_E_INVAL."""
    N = 5
    rec, x0, r_max = _recipe(pkg, N, 7, 320, 40)
    ctx.set_points_records(rec)
    for shard in ((0, 6 * N), (0, 4 * N + 1), (-1, 4), (8, 4)):
        with pytest.raises(pkg._lib.MaxCoverError) as e:
            ctx.mads_stepper(x0, r_max, 1e5, shard=shard, poll_vars="xy", **NATIVE)
        assert e.value.code == pkg._lib.MAC_E_INVAL
    for shard in ((0, 4 * N), (4 * N, 4 * N), (3, 9)):
        ctx.mads_stepper(x0, r_max, 1e5, shard=shard, poll_vars="xy", **NATIVE).close()
    # an empty shard polls nothing and says so
    s_ = ctx.mads_stepper(x0, r_max, 1e5, shard=(4, 4), poll_vars="xy", **NATIVE)
    try:
        assert s_.poll() == (False, math.inf, -1)
    finally:
        s_.close()


@pytest.mark.parametrize("mode", ["xy", "auto", "auto_in_place"])
def test_j_config1_mpc_steps(ctx, pkg, orc, firepoints, mode):
    """Config 1 (FirePoints rows, N = 5, three MPC steps; tests/test_config1.py's replay) under
    poll_vars="xy" and "auto"; auto_in_place starts with r_max a quarter above the radii, so the rule
    picks "xy"."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    N, N_iter, seed = 5, 30, 20250216
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 10 * math.tan(FOV / 2), 250.0, 250.0))
    r_max = np.full(N, 30.0 * TAN50) if mode != "auto_in_place" else x0[2 * N:] + 0.25
    sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed, r_max=r_max.copy(),
                        poll_vars="xy" if mode == "xy" else "auto")
    rec = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints[:10]])
    x_prev = x0.copy()
    d_lim = np.full(N, 10.0)
    outputs, used = [], []
    for t in (1, 2, 3):
        got = sim.step()
        if t != 1 and t + 10 - 1 < len(firepoints):
            rec = np.concatenate([rec, np.asarray(firepoints[t + 10 - 1]).reshape(-1, 5)])
        drone_locs = x_prev.copy()
        rec = rec[orc.ref_remove_covered(drone_locs, rec)]
        assert got["points"] == rec.shape[0]
        if t != 1:
            FS.r_max_update(drone_locs, r_max, N)
        single_input = drone_locs if t < 3 else outputs[-1]
        if t >= 3 and not FS.cons3_ok(x_prev, single_input, d_lim):
            single_input = drone_locs
        assert np.array_equal(got["input"], single_input)
        pv = "xy" if mode == "xy" else FS.auto_poll_vars(single_input[2 * N:], r_max)
        assert got["poll_vars"] == pv
        used.append(pv)
        c3 = TC.create_cons3(x_prev, FOV, d_lim)
        rr = r_max.copy()

        def oracle_objective(v, rec=rec, rr=rr):
            return orc.ref_objective(v, rec, rr, 1e5)

        res = TS.mads(single_input, oracle_objective, [TC.cons1, c3], N_iter=N_iter, ell0=2, ell_max=6,
                      seed=seed + t, poll_vars=pv)
        want = res.x if res.x is not None else res.i
        assert np.array_equal(sim.outputs[-1], want), t
        assert got["f"] == res.x_cost, t
        assert got["iterations"] == res.status.iteration, t
        assert got["evaluations"] == 1 + res.status.iteration * 2 * TS.polled_count(3 * N, pv), t
        assert got["feasible_evaluations"] == res.status.function_evaluations - 1, t
        if pv == "xy":
            assert want[2 * N:].tobytes() == single_input[2 * N:].tobytes()
        outputs.append(want)
        x_prev = want
    if mode == "xy":
        assert used == ["xy"] * 3
    elif mode == "auto":
        assert used[0] == "xyr"      # (radii 12 under r_max 35.75: the full poll is needed)
    else:
        assert used == ["xy"] * 3    # (in place and held there)
