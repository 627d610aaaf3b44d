"""The native MADS driver under the swarm constraints (mac_mads_run_cons / mac_mads_begin_cons,
include/maxcover.h): cons8's minimum spacing and cons7's altitude zone applied on the device to every
generated poll (k_cons.h cons_mask_gen_kernel, the prep launches' mask input).

Reference side (cases A-D, H): the Python driver TDM_STATIC_opt.mads with a plain callable objective
over the C oracle (orc.ref_objective, one trial point at a time) and the constraints as host
callables [cons8 / cons7, cons3], the recipe of test_gpu_parity.test_native_mads_matches_oracle_loop;
libmaxcover is not on that side. Every comparison is exact. The native feasible_evaluations equal
the reference's function evaluations minus the start point's. Each reference run is computed once and
shared by the modes that are compared with it."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)

_REF = {}   # (case key) -> the reference run, computed once


def _counted(c):
    """c with a rejection counter (mads() short-circuits: a constraint sees the trial points the
    ones before it passed)."""
    def f(v):
        ok = bool(c(v))
        f.rejected += not ok
        return ok
    f.rejected = 0
    f.__name__ = getattr(c, "__name__", "cons")
    return f


def _recipe(pkg, N, seed, lo, span, G=160):
    wl = pkg.workloads
    x, y, w = wl.grid_points(G)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    rng = wl.SplitMix64(seed)
    x0 = np.concatenate([np.round(lo + rng.uniform(N) * span), np.round(lo + rng.uniform(N) * span),
                         np.full(N, 36.0)])
    return rec, x0, np.full(N, 30.0 * TAN50)


def _min_pair(x0):
    N = x0.size // 3
    return min(math.sqrt((x0[i] - x0[j]) * (x0[i] - x0[j]) + (x0[N + i] - x0[N + j]) * (x0[N + i] - x0[N + j]))
               for i in range(N) for j in range(i))


def _reference(pkg, orc, key, rec, x0, r_max, swarm, mads_kw, d_lim=10.0):
    """TS.mads over the oracle's objective with [*swarm, cons3] as host callables (once per key):
    x, f, iterations, status, function evaluations, the rejections per swarm constraint, candidates
    polled."""
    if key not in _REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        N = x0.size // 3
        c3 = TC.create_cons3(x0, FOV, np.full(N, d_lim))
        cs = [_counted(c) for c in swarm]
        f0_ok = all(c(x0) for c in swarm)

        def oracle_objective(v):
            return orc.ref_objective(v, rec, r_max, 1e5)

        res = TS.mads(x0, oracle_objective, [*cs, c3], **mads_kw)
        # (the trial points each constraint rejected, the start point's own check included)
        rej = [c.rejected for c in cs]
        _REF[key] = dict(x=res.x if res.x is not None else res.i, f=res.x_cost if res.x is not None else math.inf,
                         it=res.status.iteration, limit=res.status.optimization_status == "MeshPrecisionLimit",
                         evals=res.status.function_evaluations, rejected=rej,
                         polled=res.status.iteration * 2 * x0.size, f0_ok=f0_ok, c3=c3)
    return _REF[key]


def _check(got, ref):
    xn, st = got
    assert np.array_equal(xn, ref["x"])
    assert st["f"] == ref["f"]
    assert st["iterations"] == ref["it"]
    assert (st["status"] == 0) == ref["limit"]
    assert st["feasible_evaluations"] == ref["evals"] - 1
    assert st["evaluations"] == 1 + ref["polled"]
    assert st["feasible"] == (1 if math.isfinite(ref["f"]) else 0)


def _mode(ctx, mode):
    ctx.set_algo("tiled" if mode == "tiled" else "auto")
    ctx.set_chain(mode if mode in ("five", "fused") else "auto")


MODES = ["auto", "five", "fused", "tiled"]
MADS_A = dict(N_iter=30, ell0=2, ell_max=5, seed=99)
NATIVE_A = dict(n_iter=30, ell0=2, ell_max=5, seed=99)


def _case_a(pkg, which, x0):
    TC = pkg.TDM_Constraints
    if which == "a1":
        return [TC.create_cons8(5.0)]
    if which == "a2":
        return [TC.create_cons8(6.0)]
    if which == "a3":
        N = x0.size // 3
        return [TC.create_cons8(5.0), TC.create_cons7(FOV, y_below=float(np.min(x0[N:2 * N])), h_above=30.0)]
    return [TC.create_cons8(15.0)]


def _unconstrained_a(pkg, orc):
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    return _reference(pkg, orc, "a0", rec, x0, r_max, [], MADS_A)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["a1", "a2", "a3", "a4"])
def test_a_pair_prep_pipelined(ctx, pkg, orc, which, mode):
    """N = 12 (K = 72: the poll chains, the pair prep, the pipelined loop), test_native_mads_matches_
    oracle_loop's recipe; x0's closest pair is exactly 5.0 apart. a1 starts on the strict boundary
    (feasible: 5.0 < 5.0 is false), a2 starts infeasible (f0 = +inf) and recovers, a3 adds the
    altitude zone, a4 leaves nothing feasible. Through AUTO, both forced chains and the forced
    per-candidate walk; one mask launch per poll (the prep's count)."""
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    assert _min_pair(x0) == 5.0
    swarm = _case_a(pkg, which, x0)
    ref = _reference(pkg, orc, which, rec, x0, r_max, swarm, MADS_A)
    free = _unconstrained_a(pkg, orc)
    # the reference side's own outcome (the counts the oracle gives, asserted once per mode: cheap)
    if which == "a1":
        assert ref["f0_ok"] and ref["rejected"] == [212] and ref["polled"] == 2160
        assert np.array_equal(ref["x"], free["x"]) and ref["f"] == free["f"]
        assert ref["evals"] < free["evals"]   # same iterate: the evaluation count pins the mask
    elif which == "a2":
        assert not ref["f0_ok"] and ref["f"] == 369313.77773896104
        assert not np.array_equal(ref["x"], free["x"])
    elif which == "a3":
        assert ref["rejected"] == [303, 254] and ref["f"] == 268345.6666084415
        assert not np.array_equal(ref["x"], free["x"])
    else:
        assert ref["it"] == 3 and ref["f"] == math.inf and ref["limit"] and ref["evals"] == 1
        assert np.array_equal(ref["x"], x0)
    c3 = ref["c3"]
    cons = pkg.TDM_Constraints.merge_mac_cons(swarm)[0]
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        got = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
                           cons=cons, **NATIVE_A)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        _mode(ctx, "auto")
    _check(got, ref)
    if which == "a4":
        assert got[1]["feasible_evaluations"] == 0
    # one mask launch per poll launched (the pipelined loop may have enqueued polls past the stop:
    # their mask and prep launches both return at once and both are stamped)
    assert kern.get("cons_mask_gen_kernel", 0) == kern.get("prep_kernel", 0) >= ref["it"], kern


@pytest.mark.parametrize("mode", ["auto", "five", "fused"])
@pytest.mark.parametrize("which", ["b1", "b2"])
def test_b_non_pair_prep(ctx, pkg, orc, which, mode):
    """N = 13, the same recipe: 39 % 4 != 0, so the generated poll's prep is not the pair layout.
    b1: d_sep the closest pair's exact distance sqrt(457) (strict boundary, feasible start); b2: one
    more (infeasible start)."""
    rec, x0, r_max = _recipe(pkg, 13, 2024, 320, 160)
    assert _min_pair(x0) == math.sqrt(457.0)
    d = math.sqrt(457.0) + (0.0 if which == "b1" else 1.0)
    swarm = [pkg.TDM_Constraints.create_cons8(d)]
    ref = _reference(pkg, orc, which, rec, x0, r_max, swarm, MADS_A)
    assert ref["polled"] == 2340
    if which == "b1":
        assert ref["f0_ok"] and ref["rejected"] == [830] and ref["evals"] - 1 == 1274
    else:
        assert not ref["f0_ok"] and ref["rejected"] == [1001] and ref["f"] == 289284.8888258117
    c3 = ref["c3"]
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    try:
        got = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
                           cons={"d_sep": d}, **NATIVE_A)
    finally:
        _mode(ctx, "auto")
    _check(got, ref)


def test_c_below_the_poll_chain(ctx, pkg, orc):
    """N = 5 (K = 30: the per-candidate kernel and the non-pipelined loop): the mask reaches the
    prep launch that only folds the penalty chains."""
    rec, x0, r_max = _recipe(pkg, 5, 7, 320, 40)
    d = 8.280109889280517
    ref = _reference(pkg, orc, "c5", rec, x0, r_max, [pkg.TDM_Constraints.create_cons8(d)], MADS_A)
    assert ref["polled"] == 900 and ref["rejected"] == [95] and ref["evals"] - 1 == 485
    assert ref["f"] == 114546.11108685064
    c3 = ref["c3"]
    ctx.set_points_records(rec)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        got = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
                           cons=pkg._lib.Cons(d, math.nan, math.nan), **NATIVE_A)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    _check(got, ref)
    assert kern.get("cons_mask_gen_kernel", 0) == ref["it"] - got[1]["rejected_polls"], kern
    assert "prep_kernel" not in kern   # (no poll chain at this size)


# chosen on the CPU oracle (of seeds 1..79) so that the rejected share of the N = 2 run's polls lies
# inside 5-95 %: 17 of 204 candidates
C_N2_SEED = 39


@pytest.mark.parametrize("N", [1, 2])
def test_c_one_and_two_uavs(ctx, pkg, orc, N):
    """N = 1 has no pairs: the constrained run is the unconstrained one. N = 2 starts 16 apart under
    d_sep = 15."""
    wl = pkg.workloads
    x, y, w = wl.grid_points(160)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    x0 = (np.array([400.0, 400.0, 36.0]) if N == 1
          else np.array([392.0, 408.0, 400.0, 400.0, 36.0, 36.0]))
    r_max = np.full(N, 30.0 * TAN50)
    kw = dict(N_iter=30, ell0=2, ell_max=5, seed=C_N2_SEED)
    swarm = [pkg.TDM_Constraints.create_cons8(15.0)]
    ref = _reference(pkg, orc, f"c{N}", rec, x0, r_max, swarm, kw)
    if N == 1:
        free = _reference(pkg, orc, "c1free", rec, x0, r_max, [], kw)
        assert ref["rejected"] == [0] and ref["evals"] == free["evals"]
        assert np.array_equal(ref["x"], free["x"]) and ref["f"] == free["f"]
    else:
        assert _min_pair(x0) == 16.0 and ref["f0_ok"]
        assert 0.05 * ref["polled"] <= ref["rejected"][0] <= 0.95 * ref["polled"], ref["rejected"]
    c3 = ref["c3"]
    ctx.set_points_records(rec)
    got = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
                       cons={"d_sep": 15.0}, n_iter=30, ell0=2, ell_max=5, seed=C_N2_SEED)
    _check(got, ref)
    if N == 1:
        plain = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
                             n_iter=30, ell0=2, ell_max=5, seed=C_N2_SEED)
        assert np.array_equal(got[0], plain[0]) and got[1]["f"] == plain[1]["f"]
        assert got[1]["feasible_evaluations"] == plain[1]["feasible_evaluations"]


def _lattice64():
    g = 300.0 + 17.0 * np.arange(8)
    return np.concatenate([np.tile(g, 8), np.repeat(g, 8), np.full(64, 12.0)])


@pytest.mark.parametrize("mode", ["auto", "five"])
def test_d_lattice_64(ctx, pkg, orc, mode):
    """N = 64 on an 8 x 8 lattice of pitch 17 under d_sep = 15: most candidates are rejected, the
    iterate equals the unconstrained one, so the evaluation count is the pin."""
    wl = pkg.workloads
    x, y, w = wl.grid_points(120)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    x0 = _lattice64()
    r_max = np.full(64, 12.0)
    kw = dict(N_iter=8, ell0=2, ell_max=5, seed=5)
    ref = _reference(pkg, orc, "d64", rec, x0, r_max, [pkg.TDM_Constraints.create_cons8(15.0)], kw)
    assert ref["polled"] == 3072 and ref["rejected"] == [2124] and ref["evals"] - 1 == 948
    c3 = ref["c3"]
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    try:
        args = dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, n_iter=8, ell0=2,
                    ell_max=5, seed=5)
        got = ctx.mads_run(x0, r_max, 1e5, cons={"d_sep": 15.0}, **args)
        plain = ctx.mads_run(x0, r_max, 1e5, **args)
    finally:
        _mode(ctx, "auto")
    _check(got, ref)
    assert np.array_equal(got[0], plain[0]) and got[1]["f"] == plain[1]["f"]
    assert plain[1]["feasible_evaluations"] > got[1]["feasible_evaluations"] == 948


def _jittered(pkg, N, d_sep, seed):
    """A lattice of pitch round(1.2 d_sep) jittered by at most 1 per axis: every pair starts farther
    than d_sep apart, and a poll's moves bring some closer than that."""
    rng = pkg.workloads.SplitMix64(seed)
    side = int(math.ceil(math.sqrt(N)))
    pitch = float(round(1.2 * d_sep))
    ix, iy = np.divmod(np.arange(N), side)
    jx = np.round(rng.uniform(N) * 2.0 - 1.0)
    jy = np.round(rng.uniform(N) * 2.0 - 1.0)
    return np.concatenate([100.0 + pitch * ix + jx, 100.0 + pitch * iy + jy, np.full(N, 12.0)]), side * pitch + 200.0


@pytest.mark.parametrize("N", [300, 600, 1100])
def test_e_larger_n_stepper_against_the_host_mirror(ctx, pkg, N):
    """The sizes at which the mask kernel sorts 2, 4 and 8 UAVs per thread (N = 600: two UAV blocks
    in the prep, where masked candidates are evaluated and then +inf): the native stepper under a
    mac_cons against TDM_STATIC_opt.PollStepper whose polls are the masked matrix poll
    (Context.poll_best(cons=), pinned by test_gpu_cons.py) — the build against itself: size coverage,
    not parity evidence. Same (best_obj, best_idx) per poll, same iterate."""
    TS = pkg.TDM_STATIC_opt
    d_sep = 15.0
    x0, extent = _jittered(pkg, N, d_sep, 1000 + N)
    G = int(extent // 10) + 1
    x, y, w = pkg.workloads.grid_points(G)
    ctx.set_points(x, y, w)
    r_max = np.full(N, 12.0)
    cons = {"d_sep": d_sep}
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50)
    f0, i0 = ctx.poll_best(x0[None, :], r_max, 1e5, cons=cons, **kw)
    assert i0 == 0 and math.isfinite(f0)   # the start is feasible
    masks = []

    def poll_fn(Xs):
        masks.append(ctx.cons_mask(Xs, cons))
        return ctx.poll_best(Xs, r_max, 1e5, cons=cons, **kw)

    # (mesh steps of at most 2: at 2^2 every UAV moves by up to 4 and nearly every candidate of these
    # sizes breaks the spacing somewhere)
    mirror = TS.PollStepper(x0, f0, poll_fn, N_iter=3, ell0=1, ell_max=1, seed=77)
    st = ctx.mads_stepper(x0, r_max, 1e5, n_iter=3, ell0=1, ell_max=1, seed=77, cons=cons, **kw)
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
    rejected = 1.0 - float(np.mean(np.concatenate(masks)))   # both classes occur
    assert 0.05 <= rejected <= 0.95, [1.0 - float(np.mean(m)) for m in masks]


def _a3(pkg, orc):
    rec, x0, r_max = _recipe(pkg, 12, 2024, 320, 160)
    swarm = _case_a(pkg, "a3", x0)
    ref = _reference(pkg, orc, "a3", rec, x0, r_max, swarm, MADS_A)
    c3 = ref["c3"]
    kw = dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov,
              cons=pkg.TDM_Constraints.merge_mac_cons(swarm)[0], **NATIVE_A)
    return rec, x0, r_max, ref, kw


@pytest.mark.parametrize("world", [2, 3])
def test_f_sharded_steppers(ctx, pkg, orc, world):
    """Case a3 through `world` sharded steppers in one process (test_native_mads_sharded_steppers'
    pattern): every shard's polls are masked, and every stepper ends on mads_run(cons=)'s iterate,
    objective and iteration count; the shards' feasible evaluations add up to the run's."""
    from importlib import import_module
    d = import_module(pkg.__name__ + ".dist")
    rec, x0, r_max, ref, kw = _a3(pkg, orc)
    ctx.set_points_records(rec)
    want_x, want = ctx.mads_run(x0, r_max, 1e5, **kw)
    _check((want_x, want), ref)
    K = 2 * x0.size
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=d.shard_range(K, r, world), **kw)
                for r in range(world)]
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
    assert polls == want["iterations"]
    feas = 0
    for s_ in steppers:
        xs, st = s_.result()
        s_.close()
        assert np.array_equal(xs, want_x)
        assert st["f"] == want["f"] and st["iterations"] == want["iterations"]
        assert st["evaluations"] == want["evaluations"]
        assert st["slot_fallbacks"] == 0
        feas += st["feasible_evaluations"]
    assert feas == want["feasible_evaluations"]


@pytest.mark.parametrize("world", [2, 3])
def test_f_speculative_steppers(ctx, pkg, orc, world):
    """Case a3 through the speculative loop (mac_mads_poll_ahead / mac_mads_advance): the applied
    polls' feasible counts (cons3 and the constraints) add up to mads_run(cons=)'s."""
    rec, x0, r_max, ref, kw = _a3(pkg, orc)
    ctx.set_points_records(rec)
    want_x, want = ctx.mads_run(x0, r_max, 1e5, **kw)
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, **kw) for _ in range(world)]
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
    assert useful == want["feasible_evaluations"] == ref["evals"] - 1
    for s_ in steppers:
        xs, st = s_.result()
        s_.close()
        assert np.array_equal(xs, want_x)
        assert st["f"] == want["f"] and st["iterations"] == want["iterations"]
        assert st["evaluations"] == want["evaluations"]
        assert st["slot_fallbacks"] == 0


_TIMES = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")


@pytest.mark.parametrize("N", [12, 5])
def test_g_off_is_off(pkg, N):
    """cons=None, an all-off Cons and d_sep = 0 give mads_run's outputs and statistics bit for bit
    and the same launches (no mask launch), in the pipelined loop (N = 12) and the stepper loop
    (N = 5)."""
    rec, x0, r_max = _recipe(pkg, N, 2024, 320, 160)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=TAN50, **NATIVE_A)
    runs = []
    for cons in (None, pkg._lib.Cons(math.nan, math.nan, math.nan), {"d_sep": 0.0},
                 pkg._lib.Cons(-1.0, 200.0, math.nan)):
        with pkg.Context(0) as c2:   # (fresh contexts: the same routing history)
            c2.set_points_records(rec)
            c2.profile(True)
            c2.profile_read(reset=True)
            xs, st = c2.mads_run(x0, r_max, 1e5, cons=cons, **kw)
            kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
        runs.append((xs, {k: v for k, v in st.items() if k not in _TIMES}, kern))
    for xs, st, kern in runs[1:]:
        assert np.array_equal(xs, runs[0][0])
        assert st == runs[0][1]
        assert kern == runs[0][2]
    assert "cons_mask_gen_kernel" not in runs[0][2]
    assert runs[0][1]["iterations"] > 3


def test_g_size_limit(ctx, pkg):
    """N = 2049 with a constraint on is MAC_E_INVAL at begin (the mask kernel sorts at most 2048
    UAVs in LDS); with everything off it runs."""
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
            run(cons={"d_sep": 15.0})
        assert e.value.code == pkg._lib.MAC_E_INVAL and "2048" in str(e.value)
    xs, st = ctx.mads_run(x0, r_max, 1e5, cons=pkg._lib.Cons(math.nan, math.nan, math.nan), **kw)
    assert st["iterations"] == 1 and xs.shape == x0.shape


def test_h_config1_with_the_reference_spacing(ctx, pkg, orc, firepoints):
    """tests/test_config1.py's replay, three MPC steps, with cons_ext = [create_cons8(15.0)] (the
    reference's d_sep) on both sides: FullSimulation.Simulation hands the constraint to the native
    driver; the oracle side runs it as a host callable before cons3."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    N, N_iter, seed = 5, 30, 20250216
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 10 * TAN50, 250.0, 250.0))
    assert 17.0 < _min_pair(x0) < 17.5
    sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed,
                        cons_ext=[TC.cons1, TC.create_cons8(15.0)])
    rec = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints[:10]])
    x_prev = x0.copy()
    r_max = np.full(N, 30.0 * TAN50)
    d_lim = np.full(N, 10.0)
    outputs, fs = [], []
    rejected = polled = 0
    for t in (1, 2, 3):
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
        c3 = TC.create_cons3(x_prev, FOV, d_lim)
        c8 = _counted(TC.create_cons8(15.0))
        rr = r_max.copy()

        def oracle_objective(v, rec=rec, rr=rr):
            return orc.ref_objective(v, rec, rr, 1e5)

        res = TS.mads(single_input, oracle_objective, [TC.cons1, c8, c3], N_iter=N_iter, ell0=2,
                      ell_max=6, seed=seed + t)
        want = res.x if res.x is not None else res.i
        assert np.array_equal(sim.outputs[-1], want), t
        assert got["f"] == res.x_cost, t
        assert got["iterations"] == res.status.iteration, t
        assert got["feasible_evaluations"] == res.status.function_evaluations - 1, t
        rejected += c8.rejected
        polled += res.status.iteration * 2 * x0.size
        fs.append(res.x_cost)
        outputs.append(want)
        x_prev = want
    assert (rejected, polled + 3) == (1200, 2703)   # (trial points: the polls' and the three starts)
    assert fs == [7076303.888913149, 2275553.8889131495, 272517.6666521104]
