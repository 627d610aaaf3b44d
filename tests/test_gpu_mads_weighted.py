"""GPU: the native MADS driver on lists whose weights differ: the weighted (fp64 credit row) builds of
every generated poll. csrc/eval_plan.h sets counts = poll_possible && w_uniform, and
csrc/kernel_select.h builds fiw_kernel<kCounts, kMat, kMesh>, fin2_kernel<kCounts, kMat, kXY, kMesh>
(mads_step<kXY, kMesh> in fin2's tail), shared_bits_kernel and the fp64 rows of coverage_poll_kernel /
finalize_kernel<kXY, kMesh> from it; every other driver test runs on equal weights.

The cases, lists and reference runs are tests/weighted_mads_cases.py's (checked on the CPU by
tests/test_weighted_mads_cases.py): test_gpu_poll_vars._reference (TDM_STATIC_opt.mads over
orc.ref_objective one trial point at a time, the constraints as host callables) on weights that are
multiples of 0.25, so every sum is exact and EVERY COMPARISON HERE IS == / array_equal; libmaxcover is
not on the reference side. Each reference run is computed once and shared by the chains, drivers and
key modes compared with it; where a test builds its case it asserts the case's conditions again
(successes > 3, f < f0, an iterate that is not the equal-weight run's).

Which build ran: the profile's launch counts (fiw_kernel / fin2_kernel under the forced fused chain,
coverage_poll_kernel and no fiw_kernel under the forced five-launch chain, launch role 5 for the
shared-entry pass: shared_bits_kernel on unequal weights, stamped under the role's one name
"shared_or_kernel") together with the plan of the same poll (weighted_mads_cases.assert_route:
counts == 0, kMesh 0 / 1 / 2, fused_eligible), and Context.get_points showing the list the run read.

  A  full poll, unit mesh (kMesh 0, kXY off)        D  the same on mesh keys (kMesh 2); N = 513 edges
  B  xy poll, unit mesh (kMesh 0, kXY on);          E  cons8 / motion / barrier masks over credit rows
     entries on the disks' boundaries               F  shards, speculation   G  set_regions' list
  C  value keys on a mesh (kMesh 1, kXY off / on)   H  three MPC steps of Simulation

Replacing a loaded weight by 1.0 in csrc/k_fiw.h (addresses untouched) fails, under the forced fused
chain: at fiw's whole-chunk credit test_g_regions_list (every case) and test_b_entries_on_the_boundary on
the regions list; at fiw's per-entry credit test_b_entries_on_the_boundary on the regions list (each key
mode); in fin2's shared-entry list every forced-fused case of A-E and G.
"""
from importlib import import_module

import numpy as np
import pytest

import test_gpu_granularity as tg
import test_gpu_poll_vars as tpv
import test_gpu_prog as tp
import weighted_mads_cases as wc

pytestmark = pytest.mark.gpu

CHAINS = ["five", "fused"]
DRIVERS = ["run", "stepper"]
# The layouts in a 40 x 40 square: every disk shares entries with the others. The five-launch chain
# launches its shared-entry pass of its own accord above kBitsMinDisks = 16 disks with neighbours
# ("crowded18"); at N = 12 and 16 the poll kernel's fp64 jobs take them, and Context.set_shared("bits")
# names the pass (_crowded_five runs both).
CROWDED = ("clustered", "xy16", "crowded18")


def _extra_kw(pkg, name):
    """The native keywords of a case's constraints."""
    extra = wc.CASES[name].get("extra")
    if extra == "cons8":
        return dict(cons={"d_sep": wc.D_SEP})
    if extra == "motion":
        mo = wc.motion(pkg, name)
        return dict(motion={k: mo[k] for k in ("anchor", "vel", "cone_cos", "v_max", "speed_prev", "a_max")})
    return {}


def _native_kw(pkg, name, ref):
    return dict(wc.mads_kw(name)[1], **tpv._c3kw(ref), **_extra_kw(pkg, name))


def _case(ctx, pkg, orc, name, chain, driver, lst="weighted", keys=False, shared="auto"):
    """_case_on the session's context; under mesh keys and the forced fused chain on a context of its
    own: the hint reports are kept per lane and outlive a run (fused_history_allows reads "the lane's
    last poll's report ... it may be an older poll's"), so on a used context the first reports of a run
    can be an earlier test's polls, and ident_sum == 0 is asserted of this run's alone."""
    if keys and chain == "fused":
        with pkg.Context(0) as c2:
            return _case_on(c2, pkg, orc, name, chain, driver, lst, keys, shared)
    return _case_on(ctx, pkg, orc, name, chain, driver, lst, keys, shared)


def _case_on(ctx, pkg, orc, name, chain, driver, lst="weighted", keys=False, shared="auto"):
    """One run of a case on a context: the reference's x, f, iterations, status,
    evaluations, feasible evaluations, successes and slot_fallbacks == 0; the list the run read; the
    launches and the plan of the chain that was forced. Returns (got, kern, fused hint report)."""
    ref = wc.conditions(pkg, orc, name, lst)
    x0, r_max = wc.start(pkg, name)
    kw = _native_kw(pkg, name, ref)
    N = wc.CASES[name]["N"]

    def run():
        if driver == "run":
            got = ctx.mads_run(x0, r_max, 1e5, **kw)
        else:
            got = tg._stepper_run(ctx, x0, r_max, **kw)
        return got, ctx.profile_fused(reset=True), ctx.get_points()

    try:
        if lst == "regions":   # the library makes the list: the equal-weight lattice through the override
            ctx.set_regions(*wc.REGION_BOXES, w_high=wc.W_HI)
            ctx.set_points_records(wc.records(pkg, "equal"))
        else:
            ctx.set_points_records(wc.records(pkg, lst))
        ctx.set_mesh_keys(keys)
        ctx.set_shared(shared)
        ctx.profile_fused(reset=True)
        (got, fused, pts), kern = tg._profiled(ctx, chain, run)
    finally:
        ctx.set_shared("auto")
        ctx.set_mesh_keys(False)
        if lst == "regions":
            ctx.clear_regions()
    print(name, lst, chain, driver, keys, shared, kern, fused, {k: v for k, v in got[1].items() if k not in tg._TIMES})
    rec = wc.records(pkg, lst)
    assert np.array_equal(np.stack(pts, axis=1), rec[:, [0, 1, 3]])
    assert np.unique(pts[2]).size >= 2
    wc.check(got, ref, x0, name)
    assert kern.get("prep_kernel", 0) >= ref["it"] - got[1]["rejected_polls"], kern   # the poll chain ran
    if chain == "fused":
        assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern
        wc.assert_route(pkg, name, chain, keys)
        if keys and wc.CASES[name]["gran"] is not None:
            if driver == "stepper":   # (the stepper's lane reads the hints back poll by poll)
                assert fused["reports"] > 0, fused
            assert fused["ident_sum"] == 0, fused
    if chain == "five":
        assert kern.get("coverage_poll_kernel", 0) > 0 and "fiw_kernel" not in kern and "fin2_kernel" not in kern, kern
        assert kern.get("finalize_kernel", 0) > 0, kern
        wc.assert_route(pkg, name, chain, keys)
        if name == "crowded18" or shared == "bits":
            assert name in CROWDED and kern.get(pkg._lib.PROF_ROLES[5], 0) > 0, kern   # role 5: the shared-entry pass
    if wc.CASES[name].get("extra"):
        assert kern.get("cons_mask_gen_kernel", 0) > 0, kern
    assert N == x0.size // 3
    return got, kern, fused


def _crowded_five(ctx, pkg, orc, name, chain, driver, **kw):
    """A crowded case once more under the forced five-launch chain with the shared-entry pass named."""
    if chain == "five" and name in CROWDED:
        _case(ctx, pkg, orc, name, chain, driver, shared="bits", **kw)


# ---------------------------------------------------------------- A. full poll, unit mesh

@pytest.mark.parametrize("chain", ["auto", "five", "fused"])
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("name", ["full", "clustered"])
def test_a_full_poll(ctx, pkg, orc, name, driver, chain):
    """N = 12 (K = 72: the column-triple prep), the spread and the clustered layout, mads_run (the
    pipelined loop: mads_step in fin2's tail) and the stepper, each chain: fiw_kernel<false, false, 0>,
    fin2_kernel<false, false, false, 0>; under the five-launch chain the clustered layout's shared entries
    through the poll kernel's fp64 jobs and through the shared-entry pass (shared_bits_kernel)."""
    _case(ctx, pkg, orc, name, chain, driver)
    _crowded_five(ctx, pkg, orc, name, chain, driver)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("driver", DRIVERS)
def test_a_crowded_full_poll(ctx, pkg, orc, driver, chain):
    """N = 18 in the clustered square (K = 108): more than kBitsMinDisks disks have neighbours, and the
    five-launch chain launches shared_bits_kernel (role 5) without being told to."""
    _case(ctx, pkg, orc, "crowded18", chain, driver)


# ---------------------------------------------------------------- B. xy poll

@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("driver", DRIVERS)
def test_b_xy_poll(ctx, pkg, orc, driver, chain):
    """N = 18 (K = 72, n_p = 36: the pair prep): fin2_kernel<false, false, true, 0>; the radii x0's
    bit for bit (test_gpu_poll_vars._check)."""
    got, _, _ = _case(ctx, pkg, orc, "xy18", chain, driver)
    assert got[0][36:].tobytes() == wc.start(pkg, "xy18")[0][36:].tobytes()


def test_b_xy_poll_non_pair_prep(ctx, pkg, orc):
    """N = 17 (K = 68, n_p = 34 is no multiple of 4: the non-pair prep), both chains."""
    for chain in CHAINS:
        got, _, _ = _case(ctx, pkg, orc, "xy17", chain, "run")
        assert got[0][34:].tobytes() == wc.start(pkg, "xy17")[0][34:].tobytes()


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("lst", ["weighted", "regions"])
@pytest.mark.parametrize("name,keys", [("band18", False), ("band18m", False), ("band18m", True)])
def test_b_entries_on_the_boundary(ctx, pkg, orc, name, keys, lst, chain):
    """Radii sqrt(1300.5): lattice entries within an ulp of the disks' thresholds, on the unit mesh
    and on (0.5, 0.125) under value keys and mesh keys, N = 18 on the spread layout (in the clustered
    square nearly every entry is shared and goes to fin2_kernel instead). The fp32 filter's band is entered and the
    chunk's entries are credited one by one in fp64: on the regions list in place of the whole-chunk
    credit, on the 31-weight list as the difference to the fp32 decisions. No other case enters it
    (tests/test_weighted_mads_cases.py)."""
    _case(ctx, pkg, orc, name, chain, "run", lst=lst, keys=keys)


# ---------------------------------------------------------------- C. a mesh with value keys

@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("name", ["mesh", "xy16"])
def test_c_value_keys(ctx, pkg, orc, name, driver, chain):
    """(1, 0.125) on the full poll and (0.5, 0.125) on the clustered xy poll at N = 16 (K = 64, the
    smallest xy poll that takes the chains): the kMesh = 1 builds, kXY off and on."""
    _case(ctx, pkg, orc, name, chain, driver)
    _crowded_five(ctx, pkg, orc, name, chain, driver)


# ---------------------------------------------------------------- D. mesh keys

@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("driver", DRIVERS)
@pytest.mark.parametrize("name", ["mesh", "xy16", "mesh01"])
def test_d_mesh_keys(ctx, pkg, orc, name, driver, chain):
    """The same two with set_mesh_keys(True), and (1, 0.1), where no value key packs but the mesh keys
    do: the kMesh = kMeshKeys builds; under the forced fused chain no disk off the packed keys."""
    _case(ctx, pkg, orc, name, chain, driver, keys=True)
    _crowded_five(ctx, pkg, orc, name, chain, driver, keys=True)


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("pv", ["xyr", "xy"])
def test_d_block_edges_against_value_keys(pkg, orc, pv, chain):
    """N = 513 on the weighted list (part-full prep workgroups, a second block of UAVs), (1, 0.125),
    6 iterations: mesh keys on one context against value keys on a second, byte for byte in x, f and
    the counts, both anchored to the oracle by one evaluation of the final iterate (no per-trial loop at
    this N). The xy poll (K = 2052) runs the fused chain's weighted kMeshKeys builds over two UAV blocks;
    the full poll's K = 3078 is past the fused chain's limit (kFwMaxK + 1), so there the five-launch
    chain runs under either word, which the plan and the launches both say."""
    N = 513
    name = "mesh" if pv == "xyr" else "xy16"
    gran = wc.CASES[name]["gran"]
    rec = wc.records(pkg)
    _, x0, r_max = tpv._recipe(pkg, N, 2024, 100, 600, radii=12.0)
    K = (6 if pv == "xyr" else 4) * N
    kw = dict(prev=x0, d_lim=np.full(N, 10.0), tan_half_fov=tpv.TAN50, n_iter=6, ell0=2, ell_max=5, seed=99,
              granularity=gran, poll_vars=pv)
    fused_runs = chain == "fused" and K <= 3073
    out = []
    for keys in (False, True):
        p = wc.assert_route(pkg, name, chain, keys, N=N, fused=1 if fused_runs else 0)
        assert p["mesh"] == 1 + keys and p["counts"] == 0
        with pkg.Context(0) as c2:
            c2.set_points_records(rec)
            c2.set_mesh_keys(keys)

            def run():
                got = c2.mads_run(x0, r_max, 1e5, **kw)
                return got, c2.get_points()[2]

            ((xs, st), w), kern = tg._profiled(c2, chain, run)
        assert np.unique(w).size >= 2
        assert ("fiw_kernel" in kern) == ("fin2_kernel" in kern) == fused_runs, (chain, kern)
        assert ("disk_index_kernel" in kern) == (not fused_runs), (chain, kern)
        out.append((xs, {k: v for k, v in st.items() if k not in tg._TIMES}))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1] == out[1][1]
    st = out[0][1]
    assert st["iterations"] == 6 and st["evaluations"] == 1 + 6 * K and st["slot_fallbacks"] == 0
    assert st["successes"] >= 1 and st["feasible_evaluations"] > 0
    assert st["f"] == orc.ref_objective(out[0][0], rec, r_max, 1e5)
    assert st["f"] < orc.ref_objective(x0, rec, r_max, 1e5)
    if pv == "xy":
        assert out[0][0][2 * N:].tobytes() == x0[2 * N:].tobytes()


# ---------------------------------------------------------------- E. masks over fp64 credit rows

@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name", ["cons8", "motion"])
def test_e_masks(ctx, pkg, orc, name, chain):
    """cons8 (d_sep = 5.0: x0's closest pair is exactly 5.0 apart; the reference rejects some
    candidates, not all) and cons4 / cons5 / cons6 (test_gpu_mads_motion.motion_for): dead candidates
    write 0.0 credit rows."""
    _case(ctx, pkg, orc, name, chain, "run")


@pytest.mark.parametrize("mode", CHAINS)
def test_e_progressive_barrier(ctx, pkg, orc, mode):
    """mads_run(prog=) with penalty 0 from radii 38.0: both centres are polled; test_gpu_prog's whole
    list (_run_against) and its launch counts."""
    res, rec, x0, r_max, c3 = wc.prog_conditions(pkg, orc)
    res, st, kern = tp._run_against(ctx, pkg, mode, res, rec, x0, r_max, c3, profile=True, native=wc.PROG_NATIVE)
    assert np.unique(ctx.get_points()[2]).size >= 2
    s = res.status
    assert st["two_centre_polls"] > 0 and st["slot_fallbacks"] == 0
    assert kern.get("prog_select_kernel", 0) == s.iteration, kern
    assert kern.get("prog_h_kernel", 0) == s.iteration + s.two_centre_polls - st["rejected_polls"], kern
    if mode == "fused":
        assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern
    else:
        assert kern.get("coverage_poll_kernel", 0) > 0 and "fiw_kernel" not in kern, kern


# ---------------------------------------------------------------- F. two shards and the speculative loop

@pytest.fixture
def xy16_keys(ctx, pkg, orc):
    """The xy + mesh-keys case on the session's context: (ref, x0, r_max, native keywords)."""
    ref = wc.conditions(pkg, orc, "xy16")
    x0, r_max = wc.start(pkg, "xy16")
    ctx.set_points_records(wc.records(pkg))
    ctx.set_mesh_keys(True)
    try:
        yield ref, x0, r_max, _native_kw(pkg, "xy16", ref)
    finally:
        ctx.set_mesh_keys(False)


def test_f_two_shards(ctx, pkg, orc, xy16_keys):
    """Two steppers over [0, K/2) and [K/2, K) (k0 != 0 in the second), merged by dist.reduce_best, end
    on mads_run's result and on the reference's."""
    d = import_module(pkg.__name__ + ".dist")
    ref, x0, r_max, kw = xy16_keys
    want_x, want = ctx.mads_run(x0, r_max, 1e5, **kw)
    wc.check((want_x, want), ref, x0, "xy16")
    K = wc.candidates("xy16")
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, shard=d.shard_range(K, r, 2), **kw) for r in range(2)]
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
            assert xs.tobytes() == want_x.tobytes() and np.array_equal(xs, ref["x"])
            assert {k: st[k] for k in ("f", "iterations", "evaluations", "successes")} == \
                   {k: want[k] for k in ("f", "iterations", "evaluations", "successes")}
            assert st["slot_fallbacks"] == 0
            feas += st["feasible_evaluations"]
        assert feas == want["feasible_evaluations"] == ref["evals"] - 1
    finally:
        for s_ in steppers:
            s_.close()
    assert np.unique(ctx.get_points()[2]).size >= 2


def test_f_speculation(ctx, pkg, orc, xy16_keys):
    """Two steppers in the poll_ahead / advance loop (what dist.mads_loop_speculative does after its
    gather) visit the sequential run's incumbents."""
    ref, x0, r_max, kw = xy16_keys
    steppers = [ctx.mads_stepper(x0, r_max, 1e5, **kw) for _ in range(2)]
    try:
        useful = 0
        finished = False
        while not finished:
            res = [s_.poll_ahead(j) for j, s_ in enumerate(steppers)]
            for j in range(2):
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
            assert np.array_equal(xs, ref["x"]) and xs[32:].tobytes() == x0[32:].tobytes()
            assert st["f"] == ref["f"] and st["iterations"] == ref["it"]
            assert st["evaluations"] == 1 + ref["polled"] and st["successes"] == ref["succ"]
            assert st["slot_fallbacks"] == 0
    finally:
        for s_ in steppers:
            s_.close()


def test_f_dist_loops(ctx, pkg, orc, xy16_keys):
    """dist.mads_loop and dist.mads_loop_speculative drive a stepper of the case unchanged."""
    d = import_module(pkg.__name__ + ".dist")
    ref, x0, r_max, kw = xy16_keys
    for loop in (d.mads_loop, d.mads_loop_speculative):
        st = ctx.mads_stepper(x0, r_max, 1e5, **kw)
        try:
            wc.check(loop(st), ref, x0, "xy16")
        finally:
            st.close()


# ---------------------------------------------------------------- G. the list set_regions makes

@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("name,keys", [("full", False), ("mesh", False), ("xy16", True)])
def test_g_regions_list(ctx, pkg, orc, name, keys, chain):
    """set_regions(w_high = 100) then set_points_records of the equal-weight lattice: case A's spread
    layout, case C's full poll on value keys and case D's xy layout on mesh keys against the reference on
    test_gpu_regions.ref_override's records (the device list is compared with them entry for entry).
    Whole chunks of this list share one weight: fiw_kernel's whole-chunk credit (one weight times the
    fp32 count) is taken here, which the 31-weight list never does."""
    assert name in wc.REGION_CASES
    assert 0.1 < wc.override_fraction(pkg) < 0.9
    _case(ctx, pkg, orc, name, chain, "run", lst="regions", keys=keys)


# ---------------------------------------------------------------- H. end to end

@pytest.mark.parametrize("mesh_keys", [False, True])
def test_h_simulation(ctx, pkg, orc, mesh_keys):
    """Three MPC steps of Simulation(high_interest=, poll_vars="auto", granularity=(1, 0.125), N_iter=10)
    with 16 UAVs on the default 100 x 100 DynamicArea, value keys and mesh keys: per step the device list,
    the output, f and the poll the step took equal test_gpu_regions._replay's; the first step polls every
    variable, the others the xy poll (K = 64), each on a list that holds both weights."""
    FS = pkg.FullSimulation
    D = pkg.DynamicArea.DynamicArea()
    assert D.grid_size == wc.HostArea.grid_size and D.ignition == wc.HostArea.ignition
    assert np.array_equal(D.initial_points(), wc.HostArea().initial_points())
    try:
        x0, want = wc.sim_replay(pkg, orc, D)
        ctx.set_algo("auto")
        ctx.set_chain("auto")
        ctx.profile(True)
        ctx.profile_read(reset=True)
        sim = FS.Simulation(ctx, x0, fire=D, high_interest=wc.SIM_BOXES, w_high=wc.W_HI, poll_vars="auto",
                            granularity=wc.SIM_MESH, mesh_keys=mesh_keys, **wc.SIM_KW)
        used = []
        for t in range(wc.SIM_STEPS):
            rec = sim.step()
            wt = want[t]
            gx, gy, gw = ctx.get_points()
            assert np.array_equal(np.stack([gx, gy, gw], axis=1), wt["lst"][:, [0, 1, 3]]), t
            assert set(np.unique(gw)) == {25.0, wc.W_HI}, t
            assert np.array_equal(rec["input"], wt["input"]), t
            assert np.array_equal(sim.outputs[-1], wt["x"]), t
            for k in ("t", "points", "added", "kept", "f", "poll_vars"):
                assert rec[k] == wt[k], (t, k)
            assert rec["slot_fallbacks"] == 0
            used.append(rec["poll_vars"])
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
        assert "xy" in used and "xyr" in used, used
        assert kern.get("prep_kernel", 0) > 0, kern   # (the poll chains ran)
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
        ctx.set_mesh_keys(False)
        ctx.clear_regions()
        D.close()
