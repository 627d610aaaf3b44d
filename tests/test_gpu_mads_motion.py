"""The native MADS driver under the target-motion constraints (mac_mads_run_motion /
mac_mads_begin_motion, include/maxcover.h): cons4's cone, cons5's speed and cons6's acceleration
applied on the device to every generated poll (k_cons.h cons_mask_gen_motion_kernel).

tests/test_gpu_mads_cons.py's recipe: the reference side is the Python driver TDM_STATIC_opt.mads with
a plain callable objective over the C oracle and the constraints as host callables
[cons4, cons5, cons6, cons3]; libmaxcover is not on that side. The anchor is the start point (the
previous MADS target is where the reference starts the next MADS from). The seeds of the motion data
were chosen on the CPU so that every reference run has a success and a rejection by each constraint
that is on; both are asserted. Every comparison is exact (_check: x, f, iterations, status,
feasible_evaluations, evaluations)."""
import math

import numpy as np
import pytest

from test_gpu_mads_cons import FOV, TAN50, _check, _counted, _jittered, _mode, _recipe

pytestmark = pytest.mark.gpu

NAMES = ("cons4", "cons5", "cons6")
MADS_A = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
NATIVE_A = dict(n_iter=30, ell0=2, ell_max=5, seed=99)
_REF = {}


def motion_for(pkg, x0, seed, v_max=6.0, a_max=3.0, p=(1.0, 3.0), start_rejected=False):
    """Unit velocities in random directions and speed_prev in p around the anchor x0; with
    start_rejected, UAV 0's speed_prev is a_max + 0.5, so the zero move of x0 itself violates cons6."""
    N = x0.size // 3
    rng = pkg.workloads.SplitMix64(seed)
    ang = rng.uniform(N) * 2 * math.pi
    sp = p[0] + rng.uniform(N) * (p[1] - p[0])
    if start_rejected:
        sp[0] = a_max + 0.5
    return dict(anchor=x0.copy(), vel=np.concatenate([np.cos(ang), np.sin(ang)]), speed_prev=sp,
                cone_cos=-0.5, v_max=v_max, a_max=a_max)


def host_constraints(pkg, mo, names=NAMES):
    TC = pkg.TDM_Constraints
    make = {"cons4": lambda: TC.create_cons4(mo["vel"], mo["anchor"], mo["cone_cos"]),
            "cons5": lambda: TC.create_cons5(mo["anchor"], mo["v_max"]),
            "cons6": lambda: TC.create_cons6(mo["anchor"], mo["speed_prev"], mo["a_max"])}
    return [make[n]() for n in names]


def _reference(pkg, orc, key, rec, x0, r_max, mo, mads_kw, names=NAMES, extra=()):
    """TS.mads over the oracle's objective with [*extra, *motion constraints, cons3] as host
    callables, once per key; asserts a success and a rejection by every motion constraint."""
    if key not in _REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        N = x0.size // 3
        c3 = TC.create_cons3(x0, FOV, np.full(N, 10.0))
        cs = [_counted(c) for c in host_constraints(pkg, mo, names)]

        def oracle_objective(v):
            return orc.ref_objective(v, rec, r_max, 1e5)

        res = TS.mads(x0, oracle_objective, [*extra, *cs, c3], **mads_kw)
        n_p = TS.polled_count(x0.size, mads_kw.get("poll_vars", "xyr"))
        _REF[key] = dict(x=res.x if res.x is not None else res.i,
                         f=res.x_cost if res.x is not None else math.inf, it=res.status.iteration,
                         limit=res.status.optimization_status == "MeshPrecisionLimit",
                         evals=res.status.function_evaluations, rejected=[c.rejected for c in cs],
                         polled=res.status.iteration * 2 * n_p, successes=res.status.successes, c3=c3)
        assert res.status.successes >= 1, key
        assert min(c.rejected for c in cs) >= 1, (key, [c.rejected for c in cs])
    return _REF[key]


def _native_kw(ref, mo, names=NAMES, **more):
    c3 = ref["c3"]
    keys = {"cons4": ("vel", "cone_cos"), "cons5": ("v_max",), "cons6": ("speed_prev", "a_max")}
    m = {"anchor": mo["anchor"]}
    for n in names:
        m.update({k: mo[k] for k in keys[n]})
    return dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, motion=m, **more)


def _case_a(pkg, orc):
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 3)
    return rec, x0, r_max, mo, _reference(pkg, orc, "a", rec, x0, r_max, mo, MADS_A)


@pytest.mark.parametrize("mode", ["auto", "five", "fused", "tiled"])
def test_a_all_three_through_every_chain(ctx, pkg, orc, mode):
    """N = 12 (K = 72: the poll chains, the pair prep, the pipelined loop), 30 iterations, all three
    constraints on and no mac_cons: the mask launch without the sort, one per poll."""
    rec, x0, r_max, mo, ref = _case_a(pkg, orc)
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        got = ctx.mads_run(x0, r_max, 1e5, **_native_kw(ref, mo), **NATIVE_A)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        _mode(ctx, "auto")
    _check(got, ref)
    assert kern.get("cons_mask_gen_kernel", 0) == kern.get("prep_kernel", 0) >= ref["it"], kern


@pytest.mark.parametrize("names", [("cons4",), ("cons5",), ("cons6",)])
def test_a_each_alone(ctx, pkg, orc, names):
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 3)
    ref = _reference(pkg, orc, "a-" + names[0], rec, x0, r_max, mo, MADS_A, names)
    ctx.set_points_records(rec)
    _check(ctx.mads_run(x0, r_max, 1e5, **_native_kw(ref, mo, names), **NATIVE_A), ref)


def test_a_with_the_swarm_constraints(ctx, pkg, orc):
    """All three beside cons8 and cons7 (test_gpu_mads_cons.py's case a3): the sorting kernel with the
    motion tests in its loader."""
    TC = pkg.TDM_Constraints
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 3)
    swarm = [TC.create_cons8(5.0), TC.create_cons7(FOV, y_below=float(np.min(x0[12:24])), h_above=30.0)]
    ref = _reference(pkg, orc, "a-swarm", rec, x0, r_max, mo, MADS_A, extra=swarm)
    ctx.set_points_records(rec)
    got = ctx.mads_run(x0, r_max, 1e5, cons=TC.merge_mac_cons(swarm)[0], **_native_kw(ref, mo), **NATIVE_A)
    _check(got, ref)


def test_a_start_rejected_by_cons6(ctx, pkg, orc):
    """UAV 0's speed_prev is a_max + 0.5: x0 (the zero move) violates cons6, f(x0) = +inf, and the
    first feasible candidate is a success."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 2, start_rejected=True)
    c6 = pkg.TDM_Constraints.create_cons6(mo["anchor"], mo["speed_prev"], mo["a_max"])
    assert not c6(x0)
    ref = _reference(pkg, orc, "a6", rec, x0, r_max, mo, MADS_A)
    assert math.isfinite(ref["f"])
    ctx.set_points_records(rec)
    st = ctx.mads_stepper(x0, r_max, 1e5, **_native_kw(ref, mo), **NATIVE_A)
    try:
        assert st.result()[1]["f"] == math.inf          # f(x0)
    finally:
        st.close()
    _check(ctx.mads_run(x0, r_max, 1e5, **_native_kw(ref, mo), **NATIVE_A), ref)


def test_b_below_the_poll_chain(ctx, pkg, orc):
    """N = 5 (K = 30: the per-candidate kernel and the non-pipelined loop)."""
    rec, x0, r_max = _recipe(pkg, 5, 7, 320, 40)
    mo = motion_for(pkg, x0, 1)
    ref = _reference(pkg, orc, "b5", rec, x0, r_max, mo, MADS_A)
    ctx.set_points_records(rec)
    _check(ctx.mads_run(x0, r_max, 1e5, **_native_kw(ref, mo), **NATIVE_A), ref)


def test_c_xy_only_polls(ctx, pkg, orc):
    """poll_vars="xy": the radii are held, so every move's tz is x0's (zero here)."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    mo = motion_for(pkg, x0, 2)
    ref = _reference(pkg, orc, "xy", rec, x0, r_max, mo, dict(MADS_A, poll_vars="xy"))
    ctx.set_points_records(rec)
    _check(ctx.mads_run(x0, r_max, 1e5, poll_vars="xy", **_native_kw(ref, mo), **NATIVE_A), ref)


@pytest.mark.parametrize("world", [2, 3])
def test_d_sharded_steppers(ctx, pkg, orc, world):
    from importlib import import_module
    d = import_module(pkg.__name__ + ".dist")
    rec, x0, r_max, mo, ref = _case_a(pkg, orc)
    kw = dict(_native_kw(ref, mo), **NATIVE_A)
    ctx.set_points_records(rec)
    K = 2 * x0.size
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=d.shard_range(K, r, world), **kw) for r in range(world)]
    try:
        polls = 0
        while True:
            res = [s_.poll() for s_ in steppers]
            assert len({r[0] for r in res}) == 1
            if res[0][0]:
                break
            polls += 1
            bo, bi = d.reduce_best([r[1] for r in res], [r[2] for r in res])
            for s_ in steppers:
                s_.update(bo, bi)
        assert polls == ref["it"]
        feas = 0
        for s_ in steppers:
            xs, st = s_.result()
            assert np.array_equal(xs, ref["x"]) and st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["slot_fallbacks"] == 0
            feas += st["feasible_evaluations"]
        assert feas == ref["evals"] - 1
    finally:
        for s_ in steppers:
            s_.close()


@pytest.mark.parametrize("world", [2, 3])
def test_d_speculative_steppers(ctx, pkg, orc, world):
    rec, x0, r_max, mo, ref = _case_a(pkg, orc)
    kw = dict(_native_kw(ref, mo), **NATIVE_A)
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
            assert np.array_equal(xs, ref["x"]) and st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["slot_fallbacks"] == 0
    finally:
        for s_ in steppers:
            s_.close()


def test_e_n600_stepper_against_the_host_mirror(ctx, pkg):
    """N = 600 (two UAV blocks in the prep: masked candidates are evaluated and then +inf; three UAVs
    per thread in the mask kernel): the native stepper against TDM_STATIC_opt.PollStepper whose polls
    are the masked matrix poll (Context.poll_best(motion=), pinned by test_gpu_motion.py) — the build
    against itself: size coverage. Mesh steps of at most 2: a UAV moves by 0 .. sqrt(6)."""
    TS = pkg.TDM_STATIC_opt
    N = 600
    x0, extent = _jittered(pkg, N, 15.0, 1000 + N)
    G = int(extent // 10) + 1
    x, y, w = pkg.workloads.grid_points(G)
    ctx.set_points(x, y, w)
    r_max = np.full(N, 12.0)
    mo = motion_for(pkg, x0, 5, v_max=2.2, a_max=1.0, p=(0.5, 0.5))
    mo["vel"][np.arange(2 * N) % N % 10 != 0] = 0.0      # one UAV in ten has a velocity
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50)
    f0, i0 = ctx.poll_best(x0[None, :], r_max, 1e5, motion=mo, **kw)
    assert i0 == 0 and math.isfinite(f0)
    keys = {"cons4": ("vel", "cone_cos"), "cons5": ("v_max",), "cons6": ("speed_prev", "a_max")}
    rejected = {n: 0 for n in NAMES}
    passed = [0]

    def poll_fn(Xs):
        for n in NAMES:
            one = dict({"anchor": mo["anchor"]}, **{k: mo[k] for k in keys[n]})
            rejected[n] += int((~ctx.cons_mask(Xs, None, motion=one)).sum())
        passed[0] += int(ctx.cons_mask(Xs, None, motion=mo).sum())
        return ctx.poll_best(Xs, r_max, 1e5, motion=mo, **kw)

    mirror = TS.PollStepper(x0, f0, poll_fn, N_iter=3, ell0=1, ell_max=1, seed=77)
    st = ctx.mads_stepper(x0, r_max, 1e5, n_iter=3, ell0=1, ell_max=1, seed=77, motion=mo, **kw)
    try:
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
    assert polls == 3
    assert np.array_equal(xs, xm) and stats["f"] == sm["f"]
    assert stats["f"] < f0                                   # a success
    assert min(rejected.values()) >= 1 and passed[0] >= 1, (rejected, passed)


_TIMES = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")


@pytest.mark.parametrize("N", [12, 5])
def test_f_off_is_off(pkg, N):
    """motion=None, an all-NULL Motion, NaN scalars and missing arrays give mads_run's outputs,
    statistics and launches bit for bit, with and without a mac_cons."""
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50, **NATIVE_A)
    nan = math.nan
    offs = (None, pkg._lib.Motion(), {"anchor": x0}, {"anchor": x0, "cone_cos": -0.5, "a_max": 1.0},
            dict(motion_for(pkg, x0, 1), cone_cos=nan, v_max=nan, a_max=nan))
    for cons in (None, {"d_sep": 5.0}):
        runs = []
        for m in offs:
            with pkg.Context(0) as c2:   # (fresh contexts: the same routing history)
                c2.set_points_records(rec)
                c2.profile(True)
                c2.profile_read(reset=True)
                xs, st = c2.mads_run(x0, r_max, 1e5, cons=cons, motion=m, **kw)
                kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
            runs.append((xs, {k: v for k, v in st.items() if k not in _TIMES}, kern))
        for xs, st, kern in runs[1:]:
            assert np.array_equal(xs, runs[0][0]) and st == runs[0][1] and kern == runs[0][2]
        assert ("cons_mask_gen_kernel" in runs[0][2]) == (cons is not None)


def test_f_size_limit(ctx, pkg):
    N = 2049
    x, y, w = pkg.workloads.grid_points(64)
    ctx.set_points(x, y, w)
    side = 46
    ix, iy = np.divmod(np.arange(N), side)
    x0 = np.concatenate([20.0 + 13.0 * ix, 20.0 + 13.0 * iy, np.full(N, 6.0)])
    r_max = np.full(N, 6.0)
    kw = dict(n_iter=1, ell0=1, ell_max=2, seed=3)
    for run in (lambda **k: ctx.mads_run(x0, r_max, 1e5, **kw, **k),
                lambda **k: ctx.mads_stepper(x0, r_max, 1e5, **kw, **k).close()):
        with pytest.raises(pkg._lib.MaxCoverError) as e:
            run(motion={"anchor": x0, "v_max": 2.0})
        assert e.value.code == pkg._lib.MAC_E_INVAL and "2048" in str(e.value)


def test_g_config1_simulation_against_a_host_replay(ctx, pkg, orc, firepoints):
    """tests/test_config1.py's replay, five MPC steps, with Simulation(motion=): from t = 3 on the
    native driver gets cons4 / cons5 / cons6 around the previous output (FullSimulation.derive_motion);
    the oracle side runs them as host callables before cons3, on arrays derived here by hand. Step 3
    starts from a target that moved by about 10 (speed_prev): cons6 rejects the start and every
    candidate, f stays +inf and the target stays; step 4 then has zero velocities (c = NaN)."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    N, N_iter, seed = 5, 30, 20250216
    prm = dict(cone_cos=-0.5, v_max=6.0, a_max=4.0)
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 10 * TAN50, 250.0, 250.0))
    sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed, motion=prm)
    rec = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints[:10]])
    x_prev = x0.copy()
    r_max = np.full(N, 30.0 * TAN50)
    d_lim = np.full(N, 10.0)
    outputs = []
    rejected = [0, 0, 0]
    successes = 0
    for t in (1, 2, 3, 4, 5):
        got = sim.step()
        if t != 1 and t + 10 - 1 < len(firepoints):
            rec = np.concatenate([rec, np.asarray(firepoints[t + 10 - 1]).reshape(-1, 5)])
        drone_locs = x_prev.copy()
        rec = rec[orc.ref_remove_covered(drone_locs, rec)]
        if t != 1:
            FS.r_max_update(drone_locs, r_max, N)
        single_input = drone_locs if t < 3 else outputs[-1]
        if t >= 3 and not FS.cons3_ok(x_prev, single_input, d_lim):
            single_input = drone_locs
        assert np.array_equal(got["input"], single_input)
        cs = []
        if t >= 3:
            a, b = outputs[-1], outputs[-2]
            d = a - b
            speed = np.array([math.sqrt(d[i] * d[i] + d[N + i] * d[N + i] + d[2 * N + i] * d[2 * N + i])
                              for i in range(N)])
            cs = [_counted(TC.create_cons4(d[:2 * N], a, prm["cone_cos"])),
                  _counted(TC.create_cons5(a, prm["v_max"])),
                  _counted(TC.create_cons6(a, speed, prm["a_max"]))]
        c3 = TC.create_cons3(x_prev, FOV, d_lim)
        rr = r_max.copy()

        def oracle_objective(v, rec=rec, rr=rr):
            return orc.ref_objective(v, rec, rr, 1e5)

        res = TS.mads(single_input, oracle_objective, [*cs, c3], N_iter=N_iter, ell0=2, ell_max=6,
                      seed=seed + t)
        want = res.x if res.x is not None else res.i
        assert np.array_equal(sim.outputs[-1], want), t
        assert got["f"] == res.x_cost, t
        assert got["iterations"] == res.status.iteration, t
        assert got["feasible_evaluations"] == res.status.function_evaluations - 1, t
        if cs:
            rejected = [r + c.rejected for r, c in zip(rejected, cs)]
            successes += res.status.successes
        if t == 3:
            assert res.x is None and got["f"] == math.inf and np.array_equal(want, single_input)
        outputs.append(want)
        x_prev = want
    assert min(rejected) >= 1 and successes >= 1, (rejected, successes)


def test_h_python_mads_hands_the_motion_data_to_the_device_poll(ctx, pkg, orc):
    """TDM_STATIC_opt.mads with the batched device objective: create_cons4 / 5 / 6 reach the poll as
    one mac_motion (no host callable is evaluated per candidate for them) and the run is case a's."""
    TS = pkg.TDM_STATIC_opt
    rec, x0, r_max, mo, ref = _case_a(pkg, orc)
    obj = TS.createObjective(rec, 12, r_max, ctx)
    seen = []
    poll = obj.poll

    def spy(X, cons3=None, cons=None, motion=None):
        seen.append(motion)
        return poll(X, cons3, cons, motion)

    obj.poll = spy
    cs = []
    for c in host_constraints(pkg, mo):
        cs.append(_counted(c))
        cs[-1].mac_motion = c.mac_motion          # (the counter keeps the device data)
    res = TS.mads(x0, obj, [*cs, ref["c3"]], **MADS_A)
    assert np.array_equal(res.x, ref["x"]) and res.x_cost == ref["f"]
    assert res.status.iteration == ref["it"] and res.status.successes == ref["successes"]
    assert len(seen) == ref["it"] and all(m is not None and set(m) == set(mo) for m in seen)
    assert [c.rejected for c in cs] == [0, 0, 0]      # (only x0's own check ran on the host)
