"""GPU: the progressive constraints on the device (k_prog.h; include/maxcover.h mac_prog).
Context.prog_h against the host's h bit for bit; ctx.mads_run(prog=) (mac_mads_run_prog: prog_h_kernel
in front of every poll chain, prog_select_kernel after them) against TDM_STATIC_opt.mads(cons_prog=)
over the oracle's objective, iterate for iterate; prog=None / n_cons = 0 is the call without it; three
Simulation steps against a host replay; prog_select_kernel alone on given arrays (mac_diag_prog_select)
against the rule written out in tests/prog_cases.py; the loop at N = 22 .. 600 against the host rule
over the device's own matrix poll. Every comparison is exact."""
import math
import os

import numpy as np
import pytest

import prog_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


# ---------------------------------------------------------------- prog_h

def _host_h(X, member, limit, J):
    """h of every row of X, the rule's folds run in order over i and then j, vectorised over the
    candidates and constraints only (adding +0.0 for a non-member is exact: a partial sum is +0.0,
    positive or NaN). Pinned against the scalar loop in test_host_h_helper."""
    K, N = X.shape[0], X.shape[1] // 3
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[:, 2 * N:] - limit[None, :]
        t = np.where((d > 0.0) | (d != d), d, 0.0)
        bits = ((member[:, None] >> np.arange(J, dtype=np.uint32)[None, :]) & 1).astype(bool)   # N x J
        c = np.zeros((K, J))
        for i in range(N):
            c = c + np.where(bits[i][None, :], t[:, i][:, None], 0.0)
        h = np.zeros(K)
        for j in range(J):
            h = h + c[:, j] * c[:, j]
    return h


def _h_case(N, K, J, seed):
    rng = np.random.default_rng(seed)
    limit = np.round(rng.uniform(20.0, 40.0, N) * 8) / 8
    limit[N - 1] = 0.0                        # (the underflow row below: R - limit = 2^-600 exactly)
    full = np.uint32((1 << J) - 1) if J < 32 else np.uint32(0xFFFFFFFF)
    member = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32) & full
    member[0] = full if N == 1 else 0        # a UAV in no constraint ...
    if N > 1:
        member[1] = full                      # ... and one in all of them
    X = np.empty((K, 3 * N))
    X[:, :2 * N] = rng.uniform(0, 500, (K, 2 * N))
    # radii at, one ulp above and one ulp below their limits, and up to 3 above / below
    kind = rng.integers(0, 5, (K, N))
    R = np.where(kind == 0, limit[None, :],
                 np.where(kind == 1, np.nextafter(limit, np.inf)[None, :],
                          np.where(kind == 2, np.nextafter(limit, -np.inf)[None, :],
                                   limit[None, :] + rng.uniform(-3.0, 3.0, (K, N)))))
    X[:, 2 * N:] = R
    if K >= 7:
        X[3, 2 * N + min(1, N - 1)] = math.nan                # a NaN radius of a UAV in every constraint
        X[4, 2 * N:] = limit                                   # every radius at its limit: h = 0
        X[5, 2 * N:] = np.nextafter(limit, np.inf)             # every radius one ulp above
        X[6, 2 * N:] = limit                                   # the underflow: c = 2^-600 or 0, h = 0.0
        X[6, 3 * N - 1] = 2.0 ** -600
    return X, member, limit


def test_host_h_helper(pkg):
    X, member, limit = _h_case(65, 9, 32, 5)
    want = np.array([pc.h_written_out(v, member, limit, 32) for v in X])
    assert _host_h(X, member, limit, 32).tobytes() == want.tobytes()
    TC = pkg.TDM_Constraints
    progs = [TC.create_cons1_progressive(limit)] + [TC.create_cons_progressive(i, limit) for i in (4, 9)]
    mp, plain = TC.merge_mac_prog(progs)
    assert not plain and mp["n_cons"] == 3
    via = np.array([TC.prog_h([c(v) for c in progs]) for v in X])
    assert _host_h(X, mp["member"], mp["limit"], 3).tobytes() == via.tobytes()


@pytest.mark.parametrize("N", [1, 3, 64, 65, 512, 513, 2048])
def test_prog_h_matches_the_host(ctx, pkg, N):
    """Every K and J of the issue's grid at this N (15 launches): one block of UAVs and several, K
    on each side of 8, 1 / 2 / 32 constraints."""
    nan_seen = zero_seen = pos_seen = 0
    for K in (1, 7, 8, 9, 72):
        for J in (1, 2, 32):
            X, member, limit = _h_case(N, K, J, 1000 * N + 10 * K + J)
            want = _host_h(X, member, limit, J)
            got = ctx.prog_h(X, dict(member=member, limit=limit, n_cons=J))
            assert got.tobytes() == want.tobytes(), (N, K, J, np.flatnonzero(got != want)[:5])
            nan_seen += int(np.isnan(want).sum())
            zero_seen += int((want == 0.0).sum())
            pos_seen += int((want > 0.0).sum())
    assert zero_seen and pos_seen and nan_seen


def test_prog_h_underflow_nan_and_order(ctx, pkg):
    """c = 2^-600: h = 0.0 (feasible); a NaN radius of a member: NaN, of a non-member: not; the fold's
    order over i and over j on values where reordering changes the last bit."""
    N = 3
    zeros = np.zeros(6)
    u = 2.0 ** -53
    X = np.array([np.concatenate([zeros, [2.0 ** -600, 0.0, -1.0]]),
                  np.concatenate([zeros, [1.0, u, u]]),
                  np.concatenate([zeros, [u, u, 1.0]]),
                  np.concatenate([zeros, [math.nan, 0.0, 0.0]]),
                  np.concatenate([zeros, [0.0, 0.0, math.nan]])])
    one = dict(member=np.array([1, 1, 1], dtype=np.uint32), limit=np.zeros(3), n_cons=1)
    got = ctx.prog_h(X, one)
    assert got[0] == 0.0 and got[1] == 1.0 and got[2] == (1.0 + 2.0 ** -52) ** 2
    assert math.isnan(got[3]) and math.isnan(got[4])
    part = dict(member=np.array([0, 1, 1], dtype=np.uint32), limit=np.zeros(3), n_cons=1)
    got = ctx.prog_h(X, part)
    assert got[3] == 0.0 and math.isnan(got[4])
    # over j: c = (1, a, a) with a^2 = 0.39 ulp(1): ((1 + a^2) + a^2) = 1, ((a^2 + a^2) + 1) = 1 + 2^-52
    a = 1.25 * 2.0 ** -27
    three = dict(limit=np.zeros(3), n_cons=3)
    Y = np.array([np.concatenate([zeros, [1.0, a, a]])])
    assert ctx.prog_h(Y, dict(three, member=np.array([1, 2, 4], dtype=np.uint32)))[0] == 1.0
    assert ctx.prog_h(Y, dict(three, member=np.array([4, 2, 1], dtype=np.uint32)))[0] == 1.0 + 2.0 ** -52
    # no FMA: c * c is rounded before the add
    c = 1.0 + 2.0 ** -30
    Z = np.array([np.concatenate([zeros, [1.0, c, 0.0]])])
    assert ctx.prog_h(Z, dict(member=np.array([1, 2, 0], dtype=np.uint32), limit=np.zeros(3), n_cons=2))[0] \
        == 1.0 + c * c
    assert ctx.prog_h(X, None).tobytes() == np.zeros(5).tobytes()


# ---------------------------------------------------------------- mac_mads_run_prog

NATIVE = dict(n_iter=30, ell0=2, ell_max=5, seed=99)


def _progs(pkg, N, r_max, two):
    TC = pkg.TDM_Constraints
    if two:
        return [TC.create_cons_progressive(1, r_max), TC.create_cons_progressive(2, r_max)]
    return [TC.create_cons1_progressive(r_max)]


def _reference(pkg, orc, N, radii, two, cons3, swarm_d, gran, poll_vars, h_max0=None):
    """TS.mads(cons_prog=) over the oracle's objective (penalty 0) with host callables: once per key."""
    key = (N, radii, two, cons3, swarm_d, gran, poll_vars, h_max0)
    if key not in _REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        rec, x0, r_max = pc.recipe(pkg, N, 7, 320, 40, radii) if N == 3 else pc.recipe(pkg, N, 2024, 320, 160, radii)
        c3 = TC.create_cons3(x0, pc.FOV, np.full(N, 10.0))
        ext = ([TC.create_cons8(swarm_d)] if swarm_d else []) + ([c3] if cons3 else [])
        res = TS.mads(x0, lambda v: orc.ref_objective(v, rec, r_max, 0.0), ext,
                      cons_prog=_progs(pkg, N, r_max, two), granularity=gran, poll_vars=poll_vars,
                      h_max0=h_max0, **pc.KW)
        _REF[key] = res, rec, x0, r_max, c3
    return _REF[key]


def _mode(ctx, mode):
    ctx.set_algo("auto")
    ctx.set_chain(mode if mode in ("five", "fused") else "auto")


def _run(ctx, pkg, orc, mode, N, radii, two=False, cons3=True, swarm_d=None, gran=None, poll_vars="xyr",
         h_max0=None, profile=False):
    res, rec, x0, r_max, c3 = _reference(pkg, orc, N, radii, two, cons3, swarm_d, gran, poll_vars, h_max0)
    return _run_against(ctx, pkg, mode, res, rec, x0, r_max, c3 if cons3 else None, two, swarm_d, gran, poll_vars,
                        h_max0, profile, NATIVE)


def _run_against(ctx, pkg, mode, res, rec, x0, r_max, c3, two=False, swarm_d=None, gran=None, poll_vars="xyr",
                 h_max0=None, profile=False, native=None):
    """ctx.mads_run(prog=) on (rec, x0, r_max) against the host run ``res`` of the same call: the
    whole list of what the two must share."""
    N = x0.size // 3
    mp, plain = pkg.TDM_Constraints.merge_mac_prog(_progs(pkg, N, r_max, two))
    assert not plain
    kw = dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov) if c3 is not None else {}
    if swarm_d:
        kw["cons"] = {"d_sep": swarm_d}
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    kern = None
    if profile:
        ctx.profile(True)
        ctx.profile_read(reset=True)
    try:
        xn, st = ctx.mads_run(x0, r_max, 0.0, prog=mp, h_max0=h_max0, granularity=gran, poll_vars=poll_vars,
                              **kw, **(native or NATIVE))
        if profile:
            kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        if profile:
            ctx.profile_read(reset=True)
            ctx.profile(False)
        _mode(ctx, "auto")
    s = res.status
    want_x = res.x if res.x is not None else res.i
    assert xn.tobytes() == want_x.tobytes()
    assert st["has_feasible"] == (res.x is not None) and st["has_infeasible"] == (res.i is not None)
    if res.i is None:
        assert st["x_infeasible"] is None
    else:
        assert st["x_infeasible"].tobytes() == res.i.tobytes()
        assert (st["f_infeasible"], st["h_infeasible"]) == (res.i_cost, res.i_h)
    if res.x is not None:
        assert st["f_feasible"] == res.x_cost
    assert st["f"] == (res.x_cost if res.x is not None else res.i_cost)
    assert st["h_max"] == res.h_max
    assert (st["dominating"], st["improving"], st["unsuccessful"]) == (s.dominating, s.improving, s.unsuccessful)
    assert st["two_centre_polls"] == s.two_centre_polls
    assert st["evaluated"] == s.evaluated == st["feasible_evaluations"]
    assert st["iterations"] == s.iteration and st["evaluations"] == s.function_evaluations
    assert st["successes"] == s.dominating
    assert (st["status"] == 0) == (s.optimization_status == "MeshPrecisionLimit")
    return res, st, kern


@pytest.mark.parametrize("mode", ["auto", "five", "fused"])
@pytest.mark.parametrize("radii", [36.0, 38.0])
@pytest.mark.parametrize("N", [3, 12])
def test_mads_run_prog_matches_the_host_rule(ctx, pkg, orc, N, radii, mode):
    """N = 3 (K = 18: below the poll chain) and N = 12 (K = 72: the chains), with cons3, one
    constraint over every UAV; the launches: one prog_h per polled centre, one select per iteration.
    2K <= 144 here: no thread of prog_select_kernel takes a second trip through its stride loop and
    its fourth wave holds no candidate; test_select_kernel_matches_the_rule and
    test_larger_n_run_against_the_host_rule cover the strides."""
    res, st, kern = _run(ctx, pkg, orc, mode, N, radii, profile=True)
    s = res.status
    assert s.dominating >= 1 and s.unsuccessful >= 1
    if N == 3:
        assert s.improving >= 1 and s.two_centre_polls >= 1
    assert kern.get("prog_select_kernel", 0) == s.iteration, kern
    polled = s.iteration + s.two_centre_polls - st["rejected_polls"]
    assert kern.get("prog_h_kernel", 0) == polled, kern


@pytest.mark.parametrize("N", [3, 12])
def test_two_constraints_without_cons3(ctx, pkg, orc, N):
    res, st, _ = _run(ctx, pkg, orc, "auto", N, 38.0 if N == 3 else 36.0, two=True, cons3=False)
    assert res.status.two_centre_polls >= 1


@pytest.mark.parametrize("N", [3, 12])
def test_with_cons8_the_mask_is_anded(ctx, pkg, orc, N):
    """create_cons8 beside the barrier: a candidate is left out when either rejects it. d_sep is
    chosen so that cons8 rejects some candidates and not all (the evaluated count shows both)."""
    d = 5.0 if N == 12 else 15.0
    res, st, kern = _run(ctx, pkg, orc, "auto", N, 36.0, swarm_d=d, profile=True)
    free = _reference(pkg, orc, N, 36.0, False, True, None, None, "xyr")[0]
    assert 0 < res.status.evaluated and res.status.evaluated != free.status.evaluated
    assert kern.get("cons_mask_gen_kernel", 0) == kern.get("prog_h_kernel", 0) >= 1


@pytest.mark.parametrize("N", [3, 12])
def test_on_a_mesh(ctx, pkg, orc, N):
    res, st, _ = _run(ctx, pkg, orc, "auto", N, 36.0, gran=(1.0, 0.125))
    r = res.x[2 * N:]
    assert np.any(r != np.round(r))


@pytest.mark.parametrize("N", [3, 12])
def test_xy_only_polls_launch_no_prog_h(ctx, pkg, orc, N):
    res, st, kern = _run(ctx, pkg, orc, "auto", N, 36.0, poll_vars="xy", profile=True)
    assert "prog_h_kernel" not in kern and kern.get("prog_select_kernel", 0) == res.status.iteration
    assert res.x is None and res.i is not None and res.status.improving == 0
    assert st["h_infeasible"] == st["h_max"]


def test_h_max0_given(ctx, pkg, orc):
    _run(ctx, pkg, orc, "auto", 3, 36.0, h_max0=math.inf)
    _run(ctx, pkg, orc, "auto", 12, 36.0, h_max0=20.0)


@pytest.mark.parametrize("N", [3, 12])
def test_no_prog_is_the_call_without_it(ctx, pkg, orc, N):
    _, rec, x0, r_max, c3 = _reference(pkg, orc, N, 36.0, False, True, None, None, "xyr")
    ctx.set_points_records(rec)
    kw = dict(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, **NATIVE)
    timing = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s", "slot_fallbacks")
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        base = ctx.mads_run(x0, r_max, 1e5, **kw)
        none = ctx.mads_run(x0, r_max, 1e5, prog=None, **kw)
        empty = ctx.mads_run(x0, r_max, 1e5, prog=dict(member=None, limit=None, n_cons=0), **kw)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    assert "prog_h_kernel" not in kern and "prog_select_kernel" not in kern
    for got in (none, empty):
        assert got[0].tobytes() == base[0].tobytes()
        assert {k: v for k, v in got[1].items() if k not in timing} == \
            {k: v for k, v in base[1].items() if k not in timing}
    with pytest.raises(ValueError, match="prog"):
        ctx.mads_stepper(x0, r_max, prog=dict(member=np.ones(N, dtype=np.uint32), limit=r_max, n_cons=1))


# ---------------------------------------------------------------- prog_select_kernel alone

@pytest.mark.parametrize("K", list(pc.SELECT_KS) + ["hand"])
def test_select_kernel_matches_the_rule(ctx, pkg, K):
    """Every case of prog_cases.select_cases() with this K (the hand-written ones under "hand")
    through mac_diag_prog_select, which launches prog_select_kernel as the loop does: all eight words
    of the record equal the rule written out (pinned against TDM_STATIC_opt.prog_select in
    tests/test_prog_host.py); a hand-written case also states its record. 2K <= 256: one stride trip;
    above: several, up to 52 at K = 6600; K = 63 .. 257 put the centres' border on each side of a
    wave's and of the workgroup's end."""
    cases = [c for c in pc.select_cases() if (c["want"] is not None) == (K == "hand") and K in ("hand", c["K"])]
    assert len(cases) >= 13
    for c in cases:
        want = pc.select_written_out(*pc.rule_args(c), c["obj"], c["h"], c["K"])
        if c["want"] is not None:
            assert pc.record_bytes(c["want"]) == pc.record_bytes(want), c["name"]
        got = pc.diag_prog_select(pkg, ctx, c["obj"], c["h"], c["K"], c["has_F"], c["has_I"], c["F_f"], c["I_f"],
                                  c["I_h"], c["h_max"])
        assert pc.record_bytes(got) == pc.record_bytes(want), (c["name"], got, want)


def test_select_diag_errors(ctx, pkg):
    E = pkg._lib.MAC_E_INVAL
    a = np.zeros(4)
    args = (1, 1, 0.0, 0.0, 1.0, 1.0)

    def rc(c, obj, h, K):
        return pc.diag_prog_select(pkg, c, obj, h, K, *args, check=False)

    assert rc(None, [a, None], [a, None], 4) == E                        # a null context
    for K in (0, -1, (1 << 20) + 1):                                     # K outside [1, 2^20]
        assert rc(ctx, [a, None], [a, None], K) == E
    assert rc(ctx, [a, None], [None, None], 4) == E                      # objectives without h
    assert rc(ctx, [None, None], [a, None], 4) == E                      # h without objectives
    assert rc(ctx, [a, a], [a, None], 4) == E and rc(ctx, [a, None], [a, a], 4) == E
    assert rc(ctx, [a, None], [a, None], 4) == 0 and rc(ctx, [None, a], [None, a], 4) == 0
    assert pc.diag_prog_select(pkg, ctx, [None, None], [None, None], 4, *args) == (2, math.inf, -1, 0.0, 1.0, -2, 1.0, 0)


# ---------------------------------------------------------------- the loop at N > 12

class _MatrixPollObjective:
    """The host run's objective: the device's matrix poll on a second context (penalty as the native
    run's), with .poll and .ctx so that TDM_STATIC_opt.mads_prog takes its objectives from
    Context.poll_best and its h from Context.prog_h."""

    def __init__(self, ctx2, r_max, penalty):
        self.ctx, self.r_max, self.penalty = ctx2, r_max, penalty

    def poll(self, X, *unused):
        return self.ctx.poll_best(np.asarray(X, dtype=np.float64), self.r_max, self.penalty, want_all=True)

    def __call__(self, v):
        return float(self.poll(np.asarray(v, dtype=np.float64)[None, :])[2][0])


@pytest.fixture(scope="module")
def ctx2(pkg, ctx):
    c = pkg.Context(0)
    yield c
    c.close()


def larger_n_mirror(pkg, ctx2, N, start, **over):
    """(res, rec, x0, r_max, c3, native kwargs): TDM_STATIC_opt.mads(cons_prog=) on the recipe."""
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    rec, x0, r_max, kw = pc.larger_n_recipe(pkg, N, start, **over)
    c3 = TC.create_cons3(x0, pc.FOV, np.full(N, 10.0))
    ctx2.set_points_records(rec)
    res = TS.mads(x0, _MatrixPollObjective(ctx2, r_max, 0.0), [pc.rowwise_cons3(c3)],
                  cons_prog=_progs(pkg, N, r_max, False), **kw)
    native = dict(n_iter=kw["N_iter"], ell0=kw["ell0"], ell_max=kw["ell_max"], seed=kw["seed"])
    return res, rec, x0, r_max, c3, native


@pytest.mark.parametrize("N,start", [(22, "mixed"), (43, "mixed"), (512, "mixed"), (512, "readme"), (600, "mixed")],
                         ids=["22", "43", "512", "512-readme", "600"])
def test_larger_n_run_against_the_host_rule(ctx, ctx2, pkg, N, start):
    """ctx.mads_run(prog=) against TDM_STATIC_opt.mads(cons_prog=) at the sizes the small runs leave
    out: N = 22 (2K = 264: a thread's second trip through prog_select_kernel's stride loop), 43
    (K = 258: one centre alone passes the workgroup), 512 (K = 3072, the README's size, prep_x's
    generated layout) and 600 (two UAV blocks in the prep and in prog_h_kernel: a dropped candidate is
    evaluated and then +inf; the wide index). The host run takes its objectives from the device's
    matrix poll on a second context and its h from Context.prog_h, so for f and h this is the build
    against itself (both are pinned elsewhere: against the oracle, and against the host fold in
    test_prog_h_matches_the_host): size coverage for them, and an independent check of prog_h_kernel
    on a generated source, of the mask AND, of the loop and of prog_select_kernel, whose rule the host
    runs in Python. _run_against's whole list, feasible_evaluations == evaluated included."""
    res, rec, x0, r_max, c3, native = larger_n_mirror(pkg, ctx2, N, start)
    s = res.status
    if start == "mixed":   # (the reference side: the run is no trivial one)
        assert s.two_centre_polls >= 1 and s.dominating >= 1 and s.improving + s.unsuccessful >= 1, vars(s)
        assert res.x is not None
    else:
        h0 = pkg.TDM_Constraints.prog_h([c(x0) for c in _progs(pkg, N, r_max, False)])
        assert res.x is None and s.two_centre_polls == 0 and s.improving >= 1 and res.h_max < h0, vars(s)
    assert 0 < s.evaluated < s.function_evaluations - 1   # some candidates were dropped, some not
    _run_against(ctx, pkg, "auto", res, rec, x0, r_max, c3, native=native)


# ---------------------------------------------------------------- Simulation

def test_simulation_steps_with_cons1_progressive(ctx, pkg, orc, firepoints):
    """Three MPC steps on the config-1 FirePoints list (N = 5) with cons_prog=[create_cons1_progressive]
    and penalty=0, against a host replay: the oracle's remove_covered and TS.mads(cons_prog=) over the
    oracle's objective, as tests/test_config1.py replays the plain loop."""
    FS, TS, TC = pkg.FullSimulation, pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    N, N_iter, seed = 5, 30, 20250216
    # (config 1's own start, radii 12 around (250, 250), lies on a plateau of the objective once the
    # penalty is 0: no trial point covers a fire point and nothing ever moves. This ring sits on the
    # fire with radii 30, 5.75 below r_max: the radii grow into the constraint.)
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 30.0, 255.0, 330.0))
    ctx.set_algo("auto")
    ctx.set_chain("auto")
    sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=N_iter, seed=seed,
                        cons_prog=[TC.create_cons1_progressive], penalty=0)
    rec = np.concatenate([np.asarray(r).reshape(-1, 5) for r in firepoints[:10]])
    x_prev = x0.copy()
    r_max = np.full(N, 30.0 * math.tan(pc.FOV / 2))
    d_lim = np.full(N, 10.0)
    outputs = []
    moved = both = False
    for t in (1, 2, 3):
        got = sim.step()
        if t != 1 and t + 10 - 1 < len(firepoints):
            rec = np.concatenate([rec, np.asarray(firepoints[t + 10 - 1]).reshape(-1, 5)])
        drone_locs = x_prev.copy()
        rec = rec[orc.ref_remove_covered(drone_locs, rec)]
        assert got["points"] == rec.shape[0]
        if t != 1:
            FS.r_max_update(drone_locs, r_max, N)
        assert np.array_equal(sim.r_max, r_max)
        single_input = drone_locs if t < 3 else outputs[-1]
        if t >= 3 and not FS.cons3_ok(x_prev, single_input, d_lim):
            single_input = drone_locs
        assert np.array_equal(got["input"], single_input)
        c3 = TC.create_cons3(x_prev, pc.FOV, d_lim)
        rr = r_max.copy()
        prog = TC.create_cons1_progressive(rr)
        res = TS.mads(single_input, lambda v, rec=rec, rr=rr: orc.ref_objective(v, rec, rr, 0.0),
                      [TC.cons1, c3], N_iter=N_iter, ell0=2, ell_max=6, seed=seed + t, cons_prog=[prog])
        want = res.x if res.x is not None else res.i
        assert sim.outputs[-1].tobytes() == want.tobytes(), t
        assert got["f"] == (res.x_cost if res.x is not None else res.i_cost), t
        assert got["iterations"] == res.status.iteration, t
        assert got["has_feasible"] == (res.x is not None)
        assert got["h"] == TC.prog_h([prog(want)]) and (got["h"] == 0.0) == got["has_feasible"]
        assert (got["dominating"], got["improving"], got["unsuccessful"]) == \
            (res.status.dominating, res.status.improving, res.status.unsuccessful)
        moved |= not np.array_equal(want, single_input)
        both |= res.status.two_centre_polls >= 1 and res.status.dominating >= 1 and res.status.unsuccessful >= 1
        outputs.append(want)
        x_prev = want
    assert moved and both   # (the reference side: the replay is no trivial one)
    plain = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=2, seed=seed).step()
    assert "h" not in plain and "dominating" not in plain   # (without cons_prog: the records as they were)
