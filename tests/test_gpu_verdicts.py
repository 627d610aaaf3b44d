"""GPU: constraint verdicts (include/maxcover.h mac_verdict; k_cons.h cons_explain): what rejected each
candidate, through the matrix call (mac_cons_explain_f64), the native MADS driver's tally
(MAC_OPT_VERDICTS, mac_verdict_read) and FullSimulation.Simulation(verdicts=True).

The expected records come from the host mirror TDM_Constraints.explain (tests/test_verdict_host.py pins
it against a brute force and the host callables); the cases are built, and their worth asserted, on the
CPU in tests/verdict_cases.py. The defining identity is checked against the device code that already
decides feasibility (Context.cons_mask, Context.poll_best). Every comparison is exact: integers."""
import math

import numpy as np
import pytest

import verdict_cases as vc

pytestmark = pytest.mark.gpu

KINDS = vc.KINDS


def _explain(ctx, case, C=None):
    return ctx.cons_explain(case["C"] if C is None else C, cons=case["desc"]["cons"], motion=case["desc"]["motion"],
                            prev=case["prev"], d_lim=case["d_lim"], tan_half_fov=case["tan"])


# ---------------------------------------------------------------- 1. the matrix path, record for record

@pytest.mark.parametrize("K", [1, 7])
@pytest.mark.parametrize("N", [1, 2, 12, 256, 257, 512, 513, 2048])
def test_matrix_against_the_host_mirror(ctx, pkg, N, K):
    """S = 1, 2, 4, 8 UAVs per thread and their edges, every kind on; K = 1 is candidate 5 alone (the
    one that plants the most kinds)."""
    case = vc.matrix_case(pkg, N)
    rows = slice(None) if K == 7 else slice(5, 6)
    got = _explain(ctx, case, case["C"][rows])
    assert got.dtype == pkg._lib.VERDICT_DTYPE and got.shape == (K,)
    vc.same(got, case["want"][rows])


def test_matrix_errors(ctx, pkg):
    """Reported before anything is launched: MAC_E_SIZE, N > 2048, prev without d_lim, a null output;
    K = 0 writes nothing; everything off gives the empty record without a launch."""
    L, lib = pkg.load_library(), pkg._lib
    import ctypes
    dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(lib.Verdict)
    c = np.zeros((2, 9))
    out = np.full(2, 0, dtype=lib.VERDICT_DTYPE)
    out["pairs"] = 77
    call = lambda three_n, K, prev=None, dl=None, o=out, cc=c: L.mac_cons_explain_f64(   # noqa: E731
        ctx._h, cc.ctypes.data_as(dp), three_n, K, prev, dl, 1.0, None, None,
        o.ctypes.data_as(vp) if o is not None else None)
    assert call(8, 2) == lib.MAC_E_SIZE
    big = np.zeros((1, 3 * 2049))
    assert call(3 * 2049, 1, cc=big) == lib.MAC_E_INVAL and "2048" in L.mac_last_error().decode()
    assert call(9, 2, prev=c[0].ctypes.data_as(dp)) == lib.MAC_E_INVAL
    assert call(9, 2, o=None) == lib.MAC_E_INVAL
    assert call(9, 0, o=None) == 0
    assert out["pairs"].tolist() == [77, 77]   # nothing was written so far
    assert call(9, 2) == 0
    assert out["reasons"].tolist() == [0, 0] and out["pairs"].tolist() == [0, 0]
    assert out["first_uav"].tolist() == [[-1] * 6] * 2 and not out["n_uav"].any() and not out["reserved"].any()
    assert ctx.cons_explain(np.zeros((0, 9))).shape == (0,)


# ---------------------------------------------------------------- 2. the defining identity

@pytest.mark.parametrize("N", [12, 513])
def test_identity_against_the_masks(ctx, pkg, N):
    """Kinds 1-5: bit q is the complement of cons_mask with that one constraint on; with the one kind
    on, explain gives the same bit, counts and index as with all six."""
    case = vc.matrix_case(pkg, N)
    got = _explain(ctx, case)
    for q, kind in enumerate(KINDS):
        if kind == "cons3":
            continue
        cons, motion = vc.only(case["desc"], kind)
        feasible = ctx.cons_mask(case["C"], cons, motion)
        assert np.array_equal(got["reasons"] >> q & 1 != 0, ~feasible), kind
        one = ctx.cons_explain(case["C"], cons=cons, motion=motion)
        assert np.array_equal(one["reasons"], got["reasons"] & np.uint32(1 << q)), kind
        assert np.array_equal(one["n_uav"][:, q], got["n_uav"][:, q])
        assert np.array_equal(one["first_uav"][:, q], got["first_uav"][:, q])
        assert np.array_equal(one["pairs"], got["pairs"] if kind == "cons8" else 0 * got["pairs"])


@pytest.mark.parametrize("N", [12, 513])
def test_identity_against_the_poll(ctx, pkg, N):
    """Kind 0: bit 0 against the +inf poll_best reports under prev / d_lim, on a small list."""
    case = vc.matrix_case(pkg, N)
    x, y, w = pkg.workloads.grid_points(24)
    ctx.set_points(x, y, w)
    _, _, objs = ctx.poll_best(case["C"], np.full(N, 12.0), 1e5, prev=case["prev"], d_lim=case["d_lim"],
                               tan_half_fov=case["tan"], want_all=True)
    got = ctx.cons_explain(case["C"], prev=case["prev"], d_lim=case["d_lim"], tan_half_fov=case["tan"])
    assert np.array_equal(got["reasons"] == 1, np.isinf(objs)) and 0 < np.count_nonzero(np.isinf(objs)) < len(objs)
    assert np.array_equal(got["reasons"] & ~np.uint32(1), 0 * got["reasons"])


# ---------------------------------------------------------------- 3. the sweep's edges

def test_all_coincident(ctx, pkg):
    N = 2048
    C = np.tile(np.concatenate([np.full(N, 321.0), np.full(N, -7.5), np.full(N, 2.0)]), (2, 1))
    got = ctx.cons_explain(C, cons={"d_sep": 15.0})
    for r in got:
        assert int(r["reasons"]) == 2 and int(r["pairs"]) == 2096128 == N * (N - 1) // 2
        assert r["n_uav"].tolist() == [0, N, 0, 0, 0, 0] and r["first_uav"].tolist() == [-1, 0, -1, -1, -1, -1]


def test_line_exactly_d_sep_apart(ctx, pkg):
    """600 UAVs exactly 15 apart: the line spans more than 256 d_sep, the cells are wider than the cut,
    and no pair violates the strict <."""
    C, cons = vc.line_case(pkg)
    got = ctx.cons_explain(C, cons=cons)
    vc.same(got, vc.mirror(pkg, C, cons))
    assert int(got["reasons"][0]) == 0 and int(got["pairs"][0]) == 0


def test_line_with_every_third_gap_one_ulp_short(ctx, pkg):
    C, cons = vc.line_case(pkg, shrink=True)
    got = ctx.cons_explain(C, cons=cons)
    vc.same(got, vc.mirror(pkg, C, cons))
    r = got[0]
    assert int(r["pairs"]) == 200 and int(r["n_uav"][1]) == 400 and int(r["first_uav"][1]) == 0


def test_infinite_x_is_in_no_pair(ctx, pkg):
    base = np.array([10.0, 11.0, 12.0, 13.0, 14.0, 5.0, 5.0, 5.0, 5.0, 5.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    rows = [base.copy() for _ in range(4)]
    rows[1][2] = math.inf
    rows[2][0] = -math.inf
    rows[3][7] = math.nan   # (UAV 2's y)
    C = np.array(rows)
    got = ctx.cons_explain(C, cons={"d_sep": 15.0})
    vc.same(got, vc.mirror(pkg, C, {"d_sep": 15.0}))
    assert got["pairs"].tolist() == [10, 6, 6, 6]
    assert got["n_uav"][:, 1].tolist() == [5, 4, 4, 4] and got["first_uav"][:, 1].tolist() == [0, 0, 1, 0]


def test_tiny_d_sep_without_a_cut(ctx, pkg):
    """d_sep = 1e-200: fl(d_sep^2) = 0 <= T, so the host passes dcut = +inf and every pair is tested; only
    coincident UAVs are closer."""
    N = 300
    x = 3.0 * np.arange(N)
    x[[17, 18, 200]] = x[16]      # four UAVs on one spot: 6 pairs
    x[299] = x[298]               # and one more pair
    C = np.concatenate([x, np.zeros(N), np.ones(N)])[None, :]
    got = ctx.cons_explain(C, cons={"d_sep": 1e-200})
    vc.same(got, vc.mirror(pkg, C, {"d_sep": 1e-200}))
    assert int(got["pairs"][0]) == 7 and int(got["n_uav"][0][1]) == 6 and int(got["first_uav"][0][1]) == 16


def test_ulp_ladders(ctx, pkg):
    """One ulp inside, at and outside d_sep, dlim_threshold(v_max), both of cons6's thresholds and the
    cone's cosine (the rows' own bits are stated in the helper)."""
    case = vc.ladder_case(pkg)
    got = ctx.cons_explain(case["C"], cons=case["desc"]["cons"], motion=case["desc"]["motion"])
    vc.same(got, case["want"])


# ---------------------------------------------------------------- 4. the driver's tallies

MODES = ["auto", "five", "fused", "tiled"]
_TIMES = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")


def _mode(ctx, mode):
    ctx.set_algo("tiled" if mode == "tiled" else "auto")
    ctx.set_chain(mode if mode in ("five", "fused") else "auto")


def _stats(st):
    return {k: v for k, v in st.items() if k not in _TIMES}


def _run(pkg, case, mode, on):
    """mads_run with the option on or off, in a fresh context (the same routing history for both): (x,
    stats without the timings, launches per role, the tally, the tally after that resetting read)."""
    with pkg.Context(0) as c2:
        c2.set_points_records(case["rec"])
        _mode(c2, mode)
        c2.set_verdicts(on)
        c2.profile(True)
        c2.profile_read(reset=True)
        x, st = c2.mads_run(case["x0"], case["r_max"], 1e5, **case["kw"])
        kern = {k: n for k, (ms, n) in c2.profile_kernels().items() if n}
        return x, _stats(st), kern, c2.verdict_read(reset=True), c2.verdict_read()


def _loop(steppers, reduce_best):
    while True:
        res = [s.poll() for s in steppers]
        if res[0][0]:
            break
        bo, bi = reduce_best([r[1] for r in res], [r[2] for r in res])
        for s in steppers:
            s.update(bo, bi)
    out = [s.result() for s in steppers]
    for s in steppers:
        s.close()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
def test_driver_tallies(ctx, pkg, orc, poll_vars, mode):
    """mads_run, a whole-poll stepper and a two-shard pair of steppers against the reference loop's
    non-short-circuiting counts over the launched polls; then the invariants: the option changes no
    output, statistic or profiled launch, and candidates - rejected_any is feasible_evaluations."""
    from importlib import import_module
    d = import_module(pkg.__name__ + ".dist")
    case = vc.driver_case(pkg, orc, poll_vars)
    want = case["tally"]
    ctx.set_points_records(case["rec"])
    _mode(ctx, mode)
    try:
        x_on, st_on, kern_on, tally, after = _run(pkg, case, mode, True)
        x_off, st_off, kern_off, zero, _ = _run(pkg, case, mode, False)
        # the reference: the same iterate, and the polls it counts are the polls the driver launched
        assert np.array_equal(x_on, case["x"]) and st_on["f"] == case["f"] and st_on["iterations"] == case["it"]
        assert st_on["rejected_polls"] == case["whole"]
        assert st_on["feasible_evaluations"] == case["evals"] - 1
        assert tally == want
        # option on == option off (the run ends at n_iter: no poll is enqueued past a stop, so the
        # per-role launch counts are those of the applied polls in both runs)
        assert st_on["iterations"] == case["kw"]["n_iter"]
        assert np.array_equal(x_on, x_off) and st_on == st_off and kern_on == kern_off
        assert zero == dict(candidates=0, rejected_any=0, rejected_by=dict.fromkeys(KINDS, 0), polls=0)
        assert tally["candidates"] - tally["rejected_any"] == st_on["feasible_evaluations"]
        assert after == zero   # (the read before it reset the tally)
        # a whole-poll stepper, then two shards whose tallies add up to the whole poll's
        ctx.set_verdicts(True)
        (xs, st), = _loop([ctx.mads_stepper(case["x0"], case["r_max"], 1e5, **case["kw"])], d.reduce_best)
        one = ctx.verdict_read(reset=False)
        assert one == want and np.array_equal(xs, x_on)
        assert one["candidates"] - one["rejected_any"] == st["feasible_evaluations"]
        assert ctx.verdict_read(reset=True) == one and ctx.verdict_read() == zero
        shards = [ctx.mads_stepper(case["x0"], case["r_max"], 1e5, shard=d.shard_range(case["K"], r, 2), **case["kw"])
                  for r in range(2)]
        res = _loop(shards, d.reduce_best)
        two = ctx.verdict_read(reset=True)
        assert {k: two[k] for k in ("candidates", "rejected_any", "rejected_by")} == \
               {k: want[k] for k in ("candidates", "rejected_any", "rejected_by")}
        assert two["polls"] == 2 * want["polls"]   # (tallied launches: one per stepper and poll)
        assert sum(st["feasible_evaluations"] for _, st in res) == two["candidates"] - two["rejected_any"]
        # a stepper keeps what it began with: begun with the option off, it tallies nothing
        ctx.set_verdicts(False)
        late = ctx.mads_stepper(case["x0"], case["r_max"], 1e5, **case["kw"])
        ctx.set_verdicts(True)
        _loop([late], d.reduce_best)
        assert ctx.verdict_read() == zero
    finally:
        ctx.set_verdicts(False)
        ctx.verdict_read(reset=True)
        _mode(ctx, "auto")


@pytest.mark.parametrize("mode", ["auto", "five", "tiled"])
@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
def test_a_poll_rejected_whole_is_not_tallied(ctx, pkg, orc, poll_vars, mode):
    """d_lim = 3: the first poll (step 4) is rejected whole by cons3. The pipelined loop decides that on
    the device (its explain launch returns as the chain's later launches do), the stepper on the host (no
    launch): neither tallies the poll."""
    from importlib import import_module
    d = import_module(pkg.__name__ + ".dist")
    case = vc.driver_case(pkg, orc, poll_vars, d_lim=3.0)
    assert case["whole"] >= 1
    x_on, st_on, kern_on, tally, _ = _run(pkg, case, mode, True)
    x_off, st_off, kern_off, _, _ = _run(pkg, case, mode, False)
    assert np.array_equal(x_on, case["x"]) and st_on["iterations"] == case["it"]
    assert st_on["rejected_polls"] == case["whole"]
    assert tally == case["tally"]
    assert tally["polls"] == st_on["iterations"] - st_on["rejected_polls"]
    assert tally["candidates"] - tally["rejected_any"] == st_on["feasible_evaluations"] == case["evals"] - 1
    assert np.array_equal(x_on, x_off) and st_on == st_off
    # This run stops at the mesh limit before n_iter, and the pipelined loop has by then enqueued up to
    # kMadsWindow polls past the stop, how many depending on when the host sees it; their launches return
    # at once but are stamped (tests/test_gpu_mads_cons.py test_a_pair_prep_pipelined), so the per-role
    # counts of two runs may differ by those. What holds: the same roles, each launched at least once per
    # applied poll it serves; the exact equality is test_driver_tallies', whose run ends at n_iter.
    assert st_on["iterations"] < case["kw"]["n_iter"] and set(kern_on) == set(kern_off)
    ctx.set_points_records(case["rec"])
    _mode(ctx, mode)
    ctx.set_verdicts(True)
    ctx.verdict_read(reset=True)
    try:
        (xs, st), = _loop([ctx.mads_stepper(case["x0"], case["r_max"], 1e5, **case["kw"])], d.reduce_best)
        assert ctx.verdict_read() == case["tally"] and st["rejected_polls"] == case["whole"]
    finally:
        ctx.set_verdicts(False)
        ctx.verdict_read(reset=True)
        _mode(ctx, "auto")


def test_polls_ahead_are_tallied(ctx, pkg, orc):
    """mac_mads_poll_ahead: every poll evaluated ahead is tallied, as feasible_evaluations counts them
    (steps 4, 2 and 1 under d_lim = 10: none is rejected whole). The poll 0 ahead is the reference's
    first poll."""
    case = vc.driver_case(pkg, orc, "xyr")
    ctx.set_points_records(case["rec"])
    ctx.set_verdicts(True)
    ctx.verdict_read(reset=True)
    try:
        st = ctx.mads_stepper(case["x0"], case["r_max"], 1e5, **case["kw"])
        feas = 0
        for ahead in (0, 1, 2):
            done, bo, bi, fe = st.poll_ahead(ahead)
            assert not done
            feas += fe
            if ahead == 0:
                p0 = case["polls"][0]
                t = ctx.verdict_read(reset=False)
                assert t["polls"] == 1 and t["candidates"] == case["K"] == p0.size
                assert t["rejected_any"] == np.count_nonzero(p0) and fe == np.count_nonzero(p0 == 0)
                assert t["rejected_by"] == {k: int(np.count_nonzero(p0 >> q & 1)) for q, k in enumerate(KINDS)}
        st.close()
        t = ctx.verdict_read()
        assert t["polls"] == 3 and t["candidates"] == 3 * case["K"]
        assert t["candidates"] - t["rejected_any"] == feas
    finally:
        ctx.set_verdicts(False)
        ctx.verdict_read(reset=True)


def test_prog_run_ignores_the_option(ctx, pkg, orc):
    case = vc.driver_case(pkg, orc, "xyr")
    TC = pkg.TDM_Constraints
    ctx.set_points_records(case["rec"])
    prog = TC.merge_mac_prog([TC.create_cons1_progressive(case["r_max"])], 12)[0]
    ctx.set_verdicts(True)
    ctx.verdict_read(reset=True)
    try:
        kw = dict(case["kw"], n_iter=4)
        x, st = ctx.mads_run(case["x0"], case["r_max"], 1e5, prog=prog, **kw)
        assert st["iterations"] == 4
        t = ctx.verdict_read()
        assert t == dict(candidates=0, rejected_any=0, rejected_by=dict.fromkeys(KINDS, 0), polls=0)
    finally:
        ctx.set_verdicts(False)


# ---------------------------------------------------------------- 5. Simulation(verdicts=True)

def test_simulation_records(pkg, firepoints):
    """Two MPC steps on the small fire with cons8(15.0): the per-step counts add up to the tally of a
    context that ran the same steps with the option on and never reset it; the outputs and the other
    fields equal verdicts=False."""
    FS, TC = pkg.FullSimulation, pkg.TDM_Constraints
    N = 5
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 10 * vc.TAN50, 250.0, 250.0))
    kw = dict(firepoints=firepoints, N_iter=12, seed=20250216)
    runs = {}
    for name in ("on", "off", "unreset"):
        with pkg.Context(0) as c2:
            if name == "unreset":
                c2.set_verdicts(True)
            sim = FS.Simulation(c2, x0, cons_ext=[TC.cons1, TC.create_cons8(15.0)], verdicts=name == "on", **kw)
            recs = [sim.step(), sim.step()]
            runs[name] = (recs, [o.copy() for o in sim.outputs], c2.verdict_read(reset=False))
    on, off, unreset = runs["on"], runs["off"], runs["unreset"]
    extra = {"rejected_by", "rejected_any", "polled_candidates"}
    timing = {"fire_s", "remove_s", "mads_s", "step_s", "mads_host_s"}
    for r_on, r_off, o_on, o_off in zip(on[0], off[0], on[1], off[1]):
        assert np.array_equal(o_on, o_off)
        assert set(r_on) - set(r_off) == extra and not extra & set(r_off)
        for k in set(r_off) - timing:
            assert np.array_equal(r_on[k], r_off[k]), k
        assert r_on["polled_candidates"] - r_on["rejected_any"] == r_on["feasible_evaluations"]
        assert r_on["polled_candidates"] == (r_on["iterations"] - r_on["rejected_polls"]) * 6 * N
        assert set(r_on["rejected_by"]) == set(KINDS)
        assert all(r_on["rejected_by"][k] == 0 for k in ("cons7", "cons4", "cons5", "cons6"))
    total = unreset[2]
    assert total["candidates"] == sum(r["polled_candidates"] for r in on[0]) > 0
    assert total["rejected_any"] == sum(r["rejected_any"] for r in on[0])
    assert total["rejected_by"] == {k: sum(r["rejected_by"][k] for r in on[0]) for k in KINDS}
    assert total["rejected_by"]["cons8"] > 0 and total["rejected_by"]["cons3"] > 0
    assert on[2]["candidates"] == 0 and off[2]["candidates"] == 0   # read and reset per step; never on


# ---------------------------------------------------------------- sizes beyond one block of UAVs

def _lattice(N, pitch=17.0):
    side = int(math.ceil(math.sqrt(N)))
    ix, iy = np.divmod(np.arange(N), side)
    return np.concatenate([50.0 + pitch * ix, 50.0 + pitch * iy, np.full(N, 6.0)]), side * pitch + 100.0


def test_size_limit_under_cons3_alone(ctx, pkg):
    """N = 2049 with cons3 alone: the driver runs it with the option off; with the option on the verdict
    launch could only look at 2048 UAVs, so the run and the stepper are MAC_E_INVAL when they begin. A
    prog run ignores the option, the check included."""
    N = 2049
    x0, extent = _lattice(N, 13.0)
    x, y, w = pkg.workloads.grid_points(64)
    ctx.set_points(x, y, w)
    r_max = np.full(N, 6.0)
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=vc.TAN50, n_iter=1, ell0=1, ell_max=2, seed=3)
    xs, st = ctx.mads_run(x0, r_max, 1e5, **kw)
    assert st["iterations"] == 1
    ctx.set_verdicts(True)
    ctx.verdict_read(reset=True)
    try:
        for run in (lambda: ctx.mads_run(x0, r_max, 1e5, **kw),
                    lambda: ctx.mads_stepper(x0, r_max, 1e5, **kw).close()):
            with pytest.raises(pkg._lib.MaxCoverError) as e:
                run()
            assert e.value.code == pkg._lib.MAC_E_INVAL and "2048" in str(e.value)
        plain = ctx.mads_run(x0, r_max, 1e5, **{k: v for k, v in kw.items() if k not in ("prev", "d_lim")})
        assert plain[1]["iterations"] == 1          # nothing on: nothing to explain, no limit
        assert ctx.verdict_read()["candidates"] == 0
    finally:
        ctx.set_verdicts(False)


@pytest.mark.parametrize("N", [600, 2048])
def test_tally_beyond_one_block_of_uavs(ctx, pkg, N):
    """N > 512: the prep does not decide a whole-poll rejection on the device, so the pipelined loop
    launches and tallies every applied poll (polls = iterations - rejected_polls with none rejected on
    the device); the tally's cons3 and cons8 counts are the matrix call's over the first poll, rebuilt on
    the host from the stepper's own first poll (TDM_STATIC_opt.PollStepper)."""
    TS = pkg.TDM_STATIC_opt
    x0, extent = _lattice(N)
    x, y, w = pkg.workloads.grid_points(int(extent // 10) + 1)
    ctx.set_points(x, y, w)
    r_max = np.full(N, 6.0)
    # steps of 2 on one variable and of at most 1 on the others: cons3 rejects a candidate when the UAV
    # that takes the 2 moves in another coordinate too; cons8 when a neighbour 17 away closes by 3
    d_lim = np.full(N, 2.2)
    cons = {"d_sep": 15.0}
    kw = dict(prev=x0, d_lim=d_lim, tan_half_fov=vc.TAN50, cons=cons, n_iter=2, ell0=1, ell_max=1, seed=77)
    polls = []

    def poll_fn(Xs):
        polls.append(np.array(Xs))
        return ctx.poll_best(Xs, r_max, 1e5, prev=x0, d_lim=d_lim, tan_half_fov=vc.TAN50, cons=cons)

    f0, _ = ctx.poll_best(x0[None, :], r_max, 1e5, prev=x0, d_lim=d_lim, tan_half_fov=vc.TAN50, cons=cons)
    mirror = TS.PollStepper(x0, f0, poll_fn, N_iter=2, ell0=1, ell_max=1, seed=77)
    done, bo, bi = mirror.poll()
    assert not done and len(polls) == 1 and polls[0].shape == (6 * N, 3 * N)
    want = ctx.cons_explain(polls[0], cons=cons, prev=x0, d_lim=d_lim, tan_half_fov=vc.TAN50)
    ctx.set_verdicts(True)
    ctx.verdict_read(reset=True)
    try:
        st = ctx.mads_stepper(x0, r_max, 1e5, **kw)
        got = st.poll()
        assert (got[1], got[2]) == (bo, bi)
        _, stats = st.result()
        st.close()
        t = ctx.verdict_read()
        assert t["polls"] == 1 and t["candidates"] == 6 * N
        assert t["rejected_any"] == np.count_nonzero(want["reasons"])
        assert t["rejected_by"] == {k: int(np.count_nonzero(want["reasons"] >> q & 1)) for q, k in enumerate(KINDS)}
        assert 0 < t["rejected_by"]["cons3"] < 6 * N and 0 < t["rejected_by"]["cons8"] < 6 * N
        xs, rs = ctx.mads_run(x0, r_max, 1e5, **kw)
        t = ctx.verdict_read()
        assert t["polls"] == rs["iterations"] - rs["rejected_polls"] == 2 and t["candidates"] == 2 * 6 * N
    finally:
        ctx.set_verdicts(False)
        ctx.verdict_read(reset=True)
