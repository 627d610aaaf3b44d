"""The native MADS driver on a mesh (mac_mads_run_mesh / mac_mads_begin_mesh, mac_mads_mesh;
include/maxcover.h): variable v steps by fl(g[v] * L), L the integer the stream draws on the unit
mesh, through every place a draw becomes a candidate value on the device (the prep launches, the
disk index, the constraint masks, the pipelined loop's update) and the host's updates.

Reference side: TDM_STATIC_opt.mads(granularity=) with a plain callable objective over the C oracle
(orc.ref_objective, one trial point at a time) and cons1 / cons3 (and the swarm or motion
constraints) as host callables, test_gpu_poll_vars.py's recipe; libmaxcover is not on that side
(the host mirror is pinned on the CPU by test_granularity_host.py). Every comparison is exact. Each
reference run is computed once and shared by the modes compared with it."""
import math
from importlib import import_module

import numpy as np
import pytest

from test_gpu_mads_motion import host_constraints, motion_for
from test_gpu_poll_vars import FOV, TAN50, _chain, _recipe

pytestmark = pytest.mark.gpu

MADS = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
_TIMES = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")
_REF = {}
GRANS = [(1.0, 0.1), (0.5, 0.125), (2.0, 1.0), (0.1, 0.1)]


def _native(mads_kw):
    return dict(n_iter=mads_kw["N_iter"], ell0=mads_kw["ell0"], ell_max=mads_kw["ell_max"], seed=mads_kw["seed"])


def _reference(pkg, orc, key, rec, x0, r_max, gran, extra=(), mads_kw=MADS, poll_vars="xyr"):
    if key not in _REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        N = x0.size // 3
        c3 = TC.create_cons3(x0, FOV, np.full(N, 10.0))

        def oracle_objective(v):
            return orc.ref_objective(v, rec, r_max, 1e5)

        kw = dict(mads_kw, poll_vars=poll_vars)
        if gran is not None:
            kw["granularity"] = gran
        res = TS.mads(x0, oracle_objective, [TC.cons1, *extra, c3], **kw)
        _REF[key] = dict(x=res.x if res.x is not None else res.i, f=res.x_cost if res.x is not None else math.inf,
                         it=res.status.iteration, limit=res.status.optimization_status == "MeshPrecisionLimit",
                         evals=res.status.function_evaluations, succ=res.status.successes,
                         polled=res.status.iteration * 2 * TS.polled_count(x0.size, poll_vars), c3=c3,
                         empty=res.status.cons3_empty_polls, f0=oracle_objective(x0))
    return _REF[key]


def _check(got, ref):
    xn, st = got
    assert np.array_equal(xn, ref["x"])
    assert st["f"] == ref["f"]
    assert st["iterations"] == ref["it"]
    assert (st["status"] == 0) == ref["limit"]
    assert st["evaluations"] == 1 + ref["polled"]
    assert st["feasible_evaluations"] == ref["evals"] - 1
    assert st["successes"] == ref["succ"]
    assert st["rejected_polls"] <= ref["empty"]   # (the polls with no cons3-feasible candidate: a superset)
    assert st["slot_fallbacks"] == 0


def _c3kw(ref):
    c3 = ref["c3"]
    return dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov)


def _stepper_run(ctx, x0, r_max, **kw):
    st = ctx.mads_stepper(x0, r_max, 1e5, **kw)
    try:
        while True:
            done, bo, bi = st.poll()
            if done:
                break
            assert -1 <= bi < st.candidates
            st.update(bo, bi)
        return st.result()
    finally:
        st.close()


def _profiled(ctx, chain, run):
    _chain(ctx, chain)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        got = run()
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        _chain(ctx, "auto")
    return got, kern


def _chain_reference(pkg, orc, gran, N=12):
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    ref = _reference(pkg, orc, ("chain", N, gran), rec, x0, r_max, gran)
    # the reference side's own outcome, so that no case passes trivially
    assert ref["polled"] == 30 * 6 * N and ref["succ"] >= 10 and ref["f"] < ref["f0"], (ref["succ"], ref["f"])
    r = ref["x"][2 * N:]
    if gran in ((1.0, 0.1), (0.5, 0.125)):
        assert np.count_nonzero(r != np.round(r)) >= N / 2, r
    if gran == (2.0, 1.0):
        assert np.array_equal(ref["x"], np.round(ref["x"]))
    return rec, x0, r_max, ref


@pytest.mark.parametrize("chain", ["auto", "five", "fused"])
@pytest.mark.parametrize("driver", ["run", "stepper"])
@pytest.mark.parametrize("gran", GRANS)
def test_a_chain_case(ctx, pkg, orc, gran, driver, chain):
    """N = 12 (K = 72: the poll chain; the column-triple prep): (1, 0.1) takes the identity map,
    (0.5, 0.125) fp32 keys, (2, 1) packed keys with non-unit steps, (0.1, 0.1) no exact key at all;
    mads_run (the pipelined loop) and the stepper, each chain."""
    rec, x0, r_max, ref = _chain_reference(pkg, orc, gran)
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got, kern = _profiled(ctx, chain, lambda: run(x0, r_max, 1e5, granularity=gran, **_c3kw(ref), **_native(MADS)))
    print(gran, driver, chain, kern, {k: v for k, v in got[1].items() if k not in _TIMES})
    _check(got, ref)
    assert kern.get("prep_kernel", 0) >= ref["it"] - got[1]["rejected_polls"], kern   # the poll chain ran
    if chain == "fused":
        assert kern.get("fiw_kernel", 0) > 0, kern
    if chain == "five":
        assert kern.get("coverage_poll_kernel", 0) > 0 and "fiw_kernel" not in kern, kern
    if chain == "auto" and any(g != round(g) for g in gran):
        assert "fiw_kernel" not in kern, kern   # (a fractional granularity: AUTO takes the five-launch chain)


def test_a_part_full_prep_workgroups(ctx, pkg, orc):
    """N = 13 (K = 78), (1, 0.1), under auto."""
    gran = (1.0, 0.1)
    rec, x0, r_max = _recipe(pkg, 13, 2024, 320, 160)
    ref = _reference(pkg, orc, ("chain", 13, gran), rec, x0, r_max, gran)
    assert ref["polled"] == 30 * 78 and ref["f"] < ref["f0"] and ref["succ"] >= 3
    ctx.set_points_records(rec)
    for run in (ctx.mads_run, lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k)):
        got, kern = _profiled(ctx, "auto", lambda: run(x0, r_max, 1e5, granularity=gran, **_c3kw(ref),
                                                       **_native(MADS)))
        _check(got, ref)
        assert kern.get("prep_kernel", 0) >= ref["it"] - got[1]["rejected_polls"], kern


@pytest.mark.parametrize("gran", [(1.0, 0.1), (0.5, 0.125)])
@pytest.mark.parametrize("N,seed,lo,span", [(3, 7, 320, 40), (1, 39, 400, 1)])
def test_b_below_the_chain(ctx, pkg, orc, N, seed, lo, span, gran):
    """K = 18 and 6 (the per-candidate walk and the stepper loop), 100 iterations: the runs end at
    the mesh limit."""
    mk = dict(MADS, N_iter=100)
    rec, x0, r_max = _recipe(pkg, N, seed, lo, span)
    ref = _reference(pkg, orc, ("below", N, gran), rec, x0, r_max, gran, mads_kw=mk)
    assert ref["limit"] and ref["it"] < 100 and ref["f"] < ref["f0"], (ref["it"], ref["f"])
    ctx.set_points_records(rec)
    got, kern = _profiled(ctx, "auto", lambda: ctx.mads_run(x0, r_max, 1e5, granularity=gran, **_c3kw(ref),
                                                            **_native(mk)))
    _check(got, ref)
    assert got[1]["status"] == 0 and "prep_kernel" not in kern   # (no poll chain at this size)
    _check(_stepper_run(ctx, x0, r_max, granularity=gran, **_c3kw(ref), **_native(mk)), ref)


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_c_xy_poll(ctx, pkg, orc, driver):
    """N = 12, (0.5, 0.125), poll_vars="xy": only g[0 .. 2N) is used, the radii stay x0's doubles."""
    gran = (0.5, 0.125)
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    ref = _reference(pkg, orc, "xy", rec, x0, r_max, gran, poll_vars="xy")
    assert ref["polled"] == 30 * 48 and ref["f"] < ref["f0"] and ref["succ"] >= 10
    assert np.count_nonzero(ref["x"][:24] != np.round(ref["x"][:24])) > 0   # (half steps were taken)
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, granularity=gran, poll_vars="xy", **_c3kw(ref), **_native(MADS))
    _check(got, ref)
    assert got[0][24:].tobytes() == x0[24:].tobytes()


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_d_every_poll_rejected(ctx, pkg, orc, driver):
    """g = 16 everywhere at ell0 = 0: every variable's diagonal step 16 breaks d_lim = 10 alone, so
    the one poll is rejected whole and nothing is evaluated."""
    mk = dict(MADS, ell0=0)
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    ref = _reference(pkg, orc, "rej16", rec, x0, r_max, 16.0, mads_kw=mk)
    assert ref["it"] == 1 and ref["limit"] and ref["evals"] == 1 and ref["empty"] == 1
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, granularity=16.0, **_c3kw(ref), **_native(mk))
    _check(got, ref)
    assert got[1]["rejected_polls"] == got[1]["iterations"] == 1 and got[1]["feasible_evaluations"] == 0
    assert np.array_equal(got[0], x0)


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_d_radius_columns_pass_the_rejection(ctx, pkg, orc, driver):
    """ell0 = ell_max = 4: on the unit mesh the first poll is rejected whole (every diagonal step is
    16); with (1, 0.1) a radius's diagonal step is 1.6, so no poll is."""
    mk = dict(MADS, ell0=4, ell_max=4)
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    unit = _reference(pkg, orc, "rej-unit", rec, x0, r_max, None, mads_kw=mk)
    mesh = _reference(pkg, orc, "rej-mesh", rec, x0, r_max, (1.0, 0.1), mads_kw=mk)
    assert unit["empty"] >= 1 and not np.array_equal(unit["x"], mesh["x"])
    for ref in (unit, mesh):   # (30-iteration N = 12 references)
        assert ref["succ"] >= 10 and ref["f"] < ref["f0"], (ref["succ"], ref["f"])
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, granularity=(1.0, 0.1), **_c3kw(mesh), **_native(mk))
    _check(got, mesh)
    assert got[1]["rejected_polls"] == 0
    got1 = run(x0, r_max, 1e5, granularity=1.0, **_c3kw(unit), **_native(mk))
    _check(got1, unit)
    assert got1[1]["rejected_polls"] >= 1


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_e_swarm_constraint(ctx, pkg, orc, driver):
    """create_cons8(5.0) on test_gpu_mads_cons.py's start (closest pair exactly 5.0 apart), (1, 0.1):
    the mask kernel reads the scaled candidates through the source."""
    TC = pkg.TDM_Constraints
    gran = (1.0, 0.1)
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    rejected = [0]
    c8 = TC.create_cons8(5.0)

    def counted(v):
        ok = bool(c8(v))
        rejected[0] += not ok
        return ok

    fresh = "cons8" not in _REF
    ref = _reference(pkg, orc, "cons8", rec, x0, r_max, gran, extra=[counted])
    if fresh:
        ref["rejected"] = rejected[0]
    assert 0 < ref["rejected"] < ref["polled"] and ref["f"] < ref["f0"] and ref["succ"] >= 10, (ref["succ"], ref["f"])
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, granularity=gran, cons={"d_sep": 5.0}, **_c3kw(ref), **_native(MADS))
    _check(got, ref)


@pytest.mark.parametrize("driver", ["run", "stepper"])
def test_e_motion_constraints(ctx, pkg, orc, driver):
    """cons4, cons5 and cons6 around the start (test_gpu_mads_motion.py's case a), (1, 0.1)."""
    gran = (1.0, 0.1)
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 3)
    counts = [0, 0, 0]
    hosts = host_constraints(pkg, mo)

    def wrap(i):
        def c(v):
            ok = bool(hosts[i](v))
            counts[i] += not ok
            return ok
        return c

    fresh = "motion" not in _REF
    ref = _reference(pkg, orc, "motion", rec, x0, r_max, gran, extra=[wrap(0), wrap(1), wrap(2)])
    if fresh:
        ref["rejected"] = list(counts)
    assert min(ref["rejected"]) >= 1 and ref["succ"] >= 10 and ref["f"] < ref["f0"], (ref["succ"], ref["f"])
    m = {k: mo[k] for k in ("anchor", "vel", "cone_cos", "v_max", "speed_prev", "a_max")}
    ctx.set_points_records(rec)
    run = ctx.mads_run if driver == "run" else (lambda *a, **k: _stepper_run(ctx, a[0], a[1], **k))
    got = run(x0, r_max, 1e5, granularity=gran, motion=m, **_c3kw(ref), **_native(MADS))
    _check(got, ref)


def test_f_two_shards(ctx, pkg, orc):
    """Two steppers over [0, K/2) and [K/2, K) merged by the lexicographic minimum end on the
    sequential run, (0.5, 0.125)."""
    d = import_module(pkg.__name__ + ".dist")
    gran = (0.5, 0.125)
    rec, x0, r_max, ref = _chain_reference(pkg, orc, gran)
    kw = dict(granularity=gran, **_c3kw(ref), **_native(MADS))
    ctx.set_points_records(rec)
    K = 72
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=sh, **kw) for sh in ((0, K // 2), (K // 2, K))]
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
        assert polls == ref["it"]
        feas = 0
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, ref["x"]) and st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["successes"] == ref["succ"]
            assert st["slot_fallbacks"] == 0
            feas += st["feasible_evaluations"]
        assert feas == ref["evals"] - 1
    finally:
        for s_ in steppers:
            s_.close()


def test_f_speculation(ctx, pkg, orc):
    """The poll_ahead / advance loop with ahead <= 3 (four steppers) visits the sequential run's
    incumbents, (0.5, 0.125)."""
    gran = (0.5, 0.125)
    rec, x0, r_max, ref = _chain_reference(pkg, orc, gran)
    kw = dict(granularity=gran, **_c3kw(ref), **_native(MADS))
    ctx.set_points_records(rec)
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, **kw) for _ in range(4)]
    try:
        useful = 0
        finished = False
        while not finished:
            res = [s_.poll_ahead(j) for j, s_ in enumerate(steppers)]
            for j in range(4):
                done, bo, bi, fe = res[j]
                if done:
                    finished = True
                    break
                useful += fe
                moved = [s_.advance(bo, bi) for s_ in steppers]
                assert len(set(moved)) == 1
                if moved[0]:
                    break
        assert useful == ref["evals"] - 1
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, ref["x"]) and st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["successes"] == ref["succ"]
            assert st["slot_fallbacks"] == 0
    finally:
        for s_ in steppers:
            s_.close()


def test_f_simulation_step(ctx, pkg, orc):
    """FullSimulation.Simulation(granularity=) passes the mesh to mads_run: one static step, N = 3,
    against the oracle loop."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    gran = (1.0, 0.1)
    rec, x0, r_max = _recipe(pkg, 3, 7, 320, 40)
    sim = FS.Simulation(ctx, x0, initial_points=rec, N_iter=30, seed=5, r_max=r_max.copy(), ell_max=5,
                        granularity=gran)
    got = sim.step()
    kept = rec[orc.ref_remove_covered(x0, rec)]
    c3 = TC.create_cons3(x0, FOV, np.full(3, 10.0))
    res = TS.mads(x0, lambda v: orc.ref_objective(v, kept, r_max, 1e5), [TC.cons1, c3], N_iter=30, ell0=2,
                  ell_max=5, seed=6, granularity=gran)
    assert np.array_equal(sim.outputs[-1], res.x) and got["f"] == res.x_cost
    assert got["iterations"] == res.status.iteration
    assert np.count_nonzero(res.x[6:] != np.round(res.x[6:])) >= 2


@pytest.mark.parametrize("N", [12, 5])
def test_g_off_is_off(pkg, N):
    """granularity None, 1.0 and ones(3N) give the x, f, statistics and launch counts of the call
    without the keyword, in the pipelined loop (N = 12) and the stepper loop (N = 5)."""
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50, n_iter=30, ell0=2, ell_max=5, seed=99)
    runs = []
    for extra in ({}, dict(granularity=None), dict(granularity=1.0), dict(granularity=np.ones(3 * N)),
                  dict(granularity=(1.0, 1.0), poll_vars="xyr")):
        with pkg.Context(0) as c2:   # (fresh contexts: the same routing history)
            c2.set_points_records(rec)
            c2.profile(True)
            c2.profile_read(reset=True)
            xs, st = c2.mads_run(x0, r_max, 1e5, **kw, **extra)
            kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
        runs.append((xs, {k: v for k, v in st.items() if k not in _TIMES}, kern))
    for xs, st, kern in runs[1:]:
        assert xs.tobytes() == runs[0][0].tobytes()
        assert st == runs[0][1]
        assert kern == runs[0][2]
    assert runs[0][1]["iterations"] > 3 and runs[0][1]["evaluations"] == 1 + 6 * N * runs[0][1]["iterations"]
    # the stepper likewise
    with pkg.Context(0) as c2:
        c2.set_points_records(rec)
        a = _stepper_run(c2, x0, r_max, **kw)
        b = _stepper_run(c2, x0, r_max, granularity=np.ones(3 * N), **kw)
        assert a[0].tobytes() == b[0].tobytes()
        assert {k: v for k, v in a[1].items() if k not in _TIMES} == {k: v for k, v in b[1].items() if k not in _TIMES}


def test_h_fused_hint_word_1(ctx, pkg, orc):
    """Context.profile_fused: with profiling on, the forced fused chain reports the disks that took
    one position per candidate: none with packed keys ((2, 1)), some with keys that reproduce no
    double ((1, 0.1)); nothing is counted with profiling off."""
    seen = {}
    for gran in ((2.0, 1.0), (1.0, 0.1)):
        rec, x0, r_max, ref = _chain_reference(pkg, orc, gran)
        ctx.set_points_records(rec)
        ctx.profile_fused(reset=True)
        kw = dict(granularity=gran, **_c3kw(ref), **_native(MADS))
        _chain(ctx, "fused")
        try:
            _check(_stepper_run(ctx, x0, r_max, **kw), ref)
            assert ctx.profile_fused() == {"reports": 0, "ident_sum": 0, "ident_max": 0}   # (profiling off)
            ctx.profile(True)
            _check(_stepper_run(ctx, x0, r_max, **kw), ref)
            seen[gran] = ctx.profile_fused(reset=True)
        finally:
            ctx.profile_read(reset=True)
            ctx.profile(False)
            _chain(ctx, "auto")
        assert ctx.profile_fused() == {"reports": 0, "ident_sum": 0, "ident_max": 0}
    print(seen)
    assert seen[(2.0, 1.0)]["reports"] > 0 and seen[(2.0, 1.0)]["ident_sum"] == 0
    assert seen[(1.0, 0.1)]["reports"] > 0 and 0 < seen[(1.0, 0.1)]["ident_max"] <= 12
