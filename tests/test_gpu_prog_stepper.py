"""GPU: the progressive barrier as a stepper (include/maxcover.h mac_mads_begin_prog / _poll_prog /
_advance_prog / _result_prog; DESIGN.md section 4 "Progressive barrier").

prog_part_kernel alone (mac_diag_prog_part: the stepper's own launch) over tests/prog_cases.select_cases()
and the shard splits of tests/prog_part_cases.py: the shard records merged by mac_prog_merge and finished
by the Python mirror equal the rule written out and prog_select_kernel's record on the unsplit arrays.
Context.mads_prog_stepper (the whole poll, shards, four steppers speculating) against
Context.mads_run(prog=) on the same context and against prog_cases.rule_written_out over the oracle's
objective; dist.mads_prog_loop* over RcclProgGather in a world of one; three Simulation steps with a
shard of one rank. f, h and g are selected, never summed: every comparison is exact."""
import ctypes
import math
import os
import socket
from importlib import import_module

import numpy as np
import pytest

import prog_cases as pc
import prog_part_cases as ppc

pytestmark = pytest.mark.gpu

NATIVE = dict(n_iter=30, ell0=2, ell_max=5, seed=99)
TIMING = ("seconds", "host_enqueue_s", "host_perm_s", "wait_s", "host_post_s")
_REF = {}


def _dist(pkg):
    return import_module(pkg.__name__ + ".dist")


# ---------------------------------------------------------------- prog_part_kernel alone

def diag_prog_part(pkg, ctx, case, lo, hi, tag, check=True, K=None):
    """mac_diag_prog_part (csrc/maxcover.hip; host only, not in maxcover.h): prog_part_kernel on the shard
    [lo, hi) of the case's arrays through the stepper's own launch. Returns the ProgPart."""
    lib = pkg._lib
    L = pkg.load_library()
    dp, i64 = ctypes.POINTER(ctypes.c_double), ctypes.c_int64
    L.mac_diag_prog_part.argtypes = [ctypes.c_void_p, dp, dp, dp, dp, i64, i64, i64, i64, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_double, ctypes.POINTER(lib.ProgPart)]
    L.mac_diag_prog_part.restype = ctypes.c_int32
    arrs = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64)[lo:hi])
            for a in (case["obj"][0], case["h"][0], case["obj"][1], case["h"][1])]
    ptrs = [None if a is None else a.ctypes.data_as(dp) for a in arrs]
    part = lib.ProgPart()
    rc = L.mac_diag_prog_part(None if ctx is None else ctx._h, *ptrs, hi - lo, case["K"] if K is None else K, lo, tag,
                              int(case["has_F"]), int(case["has_I"]), float(case["F_f"]), float(case["I_f"]),
                              float(case["I_h"]), float(case["h_max"]), ctypes.byref(part))
    if not check:
        return rc
    assert rc == 0, (rc, L.mac_last_error().decode())
    return part


@pytest.mark.parametrize("K", list(pc.SELECT_KS) + ["hand"])
def test_part_kernel_matches_the_rule(ctx, pkg, K):
    """Every case of this K (the hand-written ones under "hand"), whole (Kc = K: 1, 63, 64, 65, 255, 256,
    257, 3072, 6600 among them) and split into 2, 3 and 8 shards with lo > 0 and edges on the wave's and
    the workgroup's sizes; both centres, either centre null. An empty shard launches nothing: its record
    is the empty one."""
    lib, TS = pkg._lib, pkg.TDM_STATIC_opt
    picked = [(c, w, s) for c, w, s in ppc.split_cases()
              if (c["want"] is not None) == (K == "hand") and K in ("hand", c["K"])]
    assert len(picked) >= 13 and {c["centres"] for c, _, _ in picked} == {"0", "1", "both"}
    launches = 0
    for q, (c, want, splits) in enumerate(picked):
        args = pc.rule_args(c)
        sel = pc.diag_prog_select(pkg, ctx, c["obj"], c["h"], c["K"], c["has_F"], c["has_I"], c["F_f"], c["I_f"],
                                  c["I_h"], c["h_max"])
        assert pc.record_bytes(sel) == pc.record_bytes(want), (c["name"], sel, want)
        whole = None
        for shards in splits:
            parts = []
            for lo, hi in shards:
                if hi > lo:
                    parts.append(diag_prog_part(pkg, ctx, c, lo, hi, q + 1))
                    launches += 1
                else:
                    parts.append(lib.ProgPart(*TS.prog_part_empty(q + 1)))
            merged = lib.prog_merge(parts)
            assert merged.tag == q + 1
            rec = TS.prog_finish(merged.as_tuple(), *args)
            assert pc.record_bytes(rec) == pc.record_bytes(want), (c["name"], shards, rec, want)
            # the merged record itself does not depend on the partition
            whole = bytes(merged) if whole is None else whole
            assert bytes(merged) == whole, (c["name"], shards)
    assert launches >= 4 * len(picked)


def test_part_kernel_against_the_mirror_field_for_field(ctx, pkg):
    """The 96 bytes of single shards (not only what prog_finish reads of them) against
    TDM_STATIC_opt.prog_part: the hand-written cases and the first generated case of every K, the whole
    poll and the shard [65, K)."""
    TS = pkg.TDM_STATIC_opt
    seen = set()
    for c, _, _ in ppc.split_cases():
        if c["want"] is None and c["K"] in seen:
            continue
        seen.add(c["K"])
        for lo in (0, 65):
            if lo >= c["K"]:
                continue
            got = diag_prog_part(pkg, ctx, c, lo, c["K"], 3)
            want = TS.prog_part(*pc.rule_args(c), ppc.shard_cands(c, lo, c["K"]), 3)
            assert bytes(got) == ppc.part_bytes(want), (c["name"], lo, got.as_tuple(), want)


def test_part_diag_errors(ctx, pkg):
    E = pkg._lib.MAC_E_INVAL
    a = np.zeros(8)
    case = dict(obj=[a, None], h=[a, None], K=8, has_F=1, has_I=0, F_f=0.0, I_f=0.0, I_h=1.0, h_max=1.0)
    assert diag_prog_part(pkg, None, case, 0, 8, 1, check=False) == E          # a null context
    assert diag_prog_part(pkg, ctx, case, 4, 4, 1, check=False) == E           # an empty shard
    assert diag_prog_part(pkg, ctx, case, 2, 8, 1, check=False, K=7) == E      # the shard passes the poll's end
    assert diag_prog_part(pkg, ctx, dict(case, h=[None, None]), 0, 8, 1, check=False) == E
    got = diag_prog_part(pkg, ctx, dict(case, obj=[None, None], h=[None, None]), 0, 8, 9)
    assert got.as_tuple() == pkg.TDM_STATIC_opt.prog_part_empty(9)


# ---------------------------------------------------------------- the stepper

def _mode(ctx, mode):
    ctx.set_algo("auto")
    ctx.set_chain(mode if mode in ("five", "fused") else "auto")


def _problem(pkg, N, radii, seed=None):
    """(rec, x0, r_max, c3, native kwargs): tests/test_gpu_prog.py's recipes (N = 3: the host tests' own);
    radii 35.0: tests/test_prog_part_host.py's run, whose first iteration is unsuccessful and leaves an I."""
    if N == 3 or radii == 35.0:
        rec, x0, r_max = pc.recipe(pkg, N, 7, 320, 40, radii)
    else:
        rec, x0, r_max = pc.recipe(pkg, N, 2024, 320, 160, radii)
    c3 = pkg.TDM_Constraints.create_cons3(x0, pc.FOV, np.full(N, 10.0))
    return rec, x0, r_max, c3, dict(NATIVE, seed=NATIVE["seed"] if seed is None else seed)


def _kwargs(pkg, x0, r_max, c3, native, swarm_d=None, gran=None, poll_vars="xyr", h_max0=None):
    N = x0.size // 3
    mp, plain = pkg.TDM_Constraints.merge_mac_prog([pkg.TDM_Constraints.create_cons1_progressive(r_max)], N)
    assert not plain
    kw = dict(prog=mp, h_max0=h_max0, granularity=gran, poll_vars=poll_vars, **native)
    if c3 is not None:
        kw.update(prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov)
    if swarm_d:
        kw["cons"] = {"d_sep": swarm_d}
    return kw


def assert_same_native(got, want, sharded=False):
    """(x, stats) of a stepper loop against Context.mads_run(prog=)'s: x, x_infeasible, f, h, h_max and
    every count. A shard's own feasible_evaluations counts its shard only; a whole-poll stepper's is the run's."""
    (xg, sg), (xw, sw) = got, want
    assert xg.tobytes() == xw.tobytes()
    if sw["x_infeasible"] is None:
        assert sg["x_infeasible"] is None
    else:
        assert sg["x_infeasible"].tobytes() == sw["x_infeasible"].tobytes()
    skip = set(TIMING) | {"x_infeasible", "rounds"} | ({"feasible_evaluations"} if sharded else set())
    assert {k: v for k, v in sg.items() if k not in skip} == {k: v for k, v in sw.items() if k not in skip}
    assert sg["slot_fallbacks"] == 0 and sw["slot_fallbacks"] == 0


def _loops(ctx, pkg, rec, x0, r_max, kw, shard_sets, world=None, mode="auto", profile=False, spec_ahead=True):
    """Context.mads_run(prog=) and, on the same context, dist.mads_prog_loop over every shard set and
    dist.mads_prog_loop_speculative over ``world`` steppers. Returns (the run, per-set results, the
    speculative result and its rounds, kernel counts of the first set)."""
    d = _dist(pkg)
    ctx.set_points_records(rec)
    _mode(ctx, mode)
    kern = None
    try:
        want = ctx.mads_run(x0, r_max, 0.0, **kw)
        outs = []
        for q, shards in enumerate(shard_sets):
            st = [ctx.mads_prog_stepper(x0, r_max, 0.0, shard=sh, **kw) for sh in shards]
            if profile and q == 0:
                ctx.profile(True)
                ctx.profile_read(reset=True)
            try:
                (x, stats), _ = ppc.lock_step(st, d.mads_prog_loop)
                if profile and q == 0:
                    kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
                outs.append((x, stats))
                assert_same_native((x, stats), want, sharded=len(shards) > 1)
                fe = stats["feasible_evaluations"]
                for s in st[1:]:
                    other = s.result()
                    assert_same_native(other, want, sharded=True)
                    fe += other[1]["feasible_evaluations"]
                assert fe == want[1]["feasible_evaluations"] == want[1]["evaluated"]
            finally:
                if profile and q == 0:
                    ctx.profile_read(reset=True)
                    ctx.profile(False)
                for s in st:
                    s.close()
        spec = None
        if world:
            st = [ctx.mads_prog_stepper(x0, r_max, 0.0, **kw) for _ in range(world)]
            try:
                (x, stats), rounds = ppc.lock_step(st, d.mads_prog_loop_speculative, ahead=True)
                assert_same_native((x, stats), want, sharded=True)   # (its polls ahead count as evaluations of its own)
                assert stats["rounds"] == len(rounds) and sum(rounds) == want[1]["iterations"]
                spec = (x, stats), rounds
            finally:
                for s in st:
                    s.close()
    finally:
        _mode(ctx, "auto")
    return want, outs, spec, kern


def _host_rule(pkg, orc, N, radii, seed=None):
    """prog_cases.rule_written_out over the oracle's objective with cons3: once per key."""
    key = (N, radii, seed)
    if key not in _REF:
        rec, x0, r_max, c3, native = _problem(pkg, N, radii, seed)
        _REF[key] = pc.rule_written_out(pkg, lambda v: orc.ref_objective(v, rec, r_max, 0.0), [c3], [1] * N, r_max, 1,
                                        x0, None, x0.size, N_iter=native["n_iter"], ell0=native["ell0"],
                                        ell_max=native["ell_max"], seed=native["seed"])
    return _REF[key]


def assert_matches_host_rule(got, want):
    x, st = got
    F, I = want["F"], want["I"]
    assert x.tobytes() == (F[0] if F is not None else I[0]).tobytes()
    assert st["has_feasible"] == (F is not None) and st["has_infeasible"] == (I is not None)
    if I is not None:
        assert st["x_infeasible"].tobytes() == I[0].tobytes()
        assert (st["f_infeasible"], st["h_infeasible"]) == (I[1], I[2])
    if F is not None:
        assert st["f_feasible"] == F[1]
    assert st["h_max"] == want["h_max"]
    assert (st["dominating"], st["improving"], st["unsuccessful"]) == \
        (want["dominating"], want["improving"], want["unsuccessful"])
    assert st["two_centre_polls"] == want["two"] and st["evaluated"] == want["evaluated"]
    assert st["iterations"] == want["it"] and st["evaluations"] == want["evals"]


@pytest.mark.parametrize("mode", ["auto", "five", "fused"])
@pytest.mark.parametrize("radii", [36.0, 38.0])
@pytest.mark.parametrize("N", [3, 12])
def test_stepper_matches_the_run_and_the_host_rule(ctx, pkg, orc, N, radii, mode):
    """K = 18 and 72: the whole poll, two shards (below kPollMinK: the small-batch path) and three shards
    with one empty, under every chain. One prog_h launch per polled centre and shard, one prog_part launch
    per poll that polled a centre (under prog_select_kernel's role; no prog_select launch)."""
    rec, x0, r_max, c3, native = _problem(pkg, N, radii)
    K = 6 * N
    sets = [[None], [(0, K // 2), (K // 2, K)], [(0, 5), (5, 5), (5, K)]]
    want, outs, _, kern = _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native), sets, mode=mode,
                                 profile=True)
    rule = _host_rule(pkg, orc, N, radii)
    assert rule["dominating"] >= 1 and rule["unsuccessful"] >= 1
    for got in outs:
        assert_matches_host_rule(got, rule)
    st = want[1]
    polled = st["iterations"] + st["two_centre_polls"] - st["rejected_polls"]
    assert kern.get("prog_h_kernel", 0) == polled, kern
    assert 1 <= kern.get("prog_select_kernel", 0) <= st["iterations"], kern


@pytest.mark.parametrize("shards", [[(0, 66), (66, 132)], [(0, 64), (64, 132)]], ids=["even", "uneven"])
def test_n22_each_shard_runs_a_chain(ctx, pkg, shards):
    rec, x0, r_max, kw = pc.larger_n_recipe(pkg, 22)
    c3 = pkg.TDM_Constraints.create_cons3(x0, pc.FOV, np.full(22, 10.0))
    native = dict(n_iter=kw["N_iter"], ell0=kw["ell0"], ell_max=kw["ell_max"], seed=kw["seed"])
    want, _, _, _ = _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native), [shards])
    assert want[1]["two_centre_polls"] >= 1 and want[1]["dominating"] >= 1


def test_n600_two_shards_against_the_run(ctx, pkg):
    """N = 600: two UAV blocks of prog_h_kernel, K = 3600, the shard's offset in a wide poll. Against
    Context.mads_run(prog=) only (the build against itself: tests/test_gpu_prog.py
    test_larger_n_run_against_the_host_rule pins that side)."""
    rec, x0, r_max, kw = pc.larger_n_recipe(pkg, 600)
    c3 = pkg.TDM_Constraints.create_cons3(x0, pc.FOV, np.full(600, 10.0))
    native = dict(n_iter=kw["N_iter"], ell0=kw["ell0"], ell_max=kw["ell_max"], seed=kw["seed"])
    want, _, _, _ = _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native), [[(0, 1800), (1800, 3600)]])
    assert want[1]["two_centre_polls"] >= 1 and want[1]["dominating"] >= 1


def test_with_cons8_on_a_mesh_xy_only_and_h_max0(ctx, pkg):
    """One case each, two shards: cons8 beside the barrier (the mask AND), granularity (1, 0.125),
    poll_vars="xy" (no prog_h_kernel launch) and a given h_max0."""
    rec, x0, r_max, c3, native = _problem(pkg, 12, 36.0)
    sets = [[(0, 36), (36, 72)]]
    _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native, swarm_d=5.0), sets)
    _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native, gran=(1.0, 0.125)), sets)
    _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native, h_max0=20.0), sets)
    want, _, _, kern = _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native, poll_vars="xy"),
                              [[(0, 24), (24, 48)]], profile=True)
    assert "prog_h_kernel" not in kern and kern.get("prog_select_kernel", 0) >= 1
    assert want[1]["improving"] == 0 and want[1]["h_infeasible"] == want[1]["h_max"]


@pytest.mark.parametrize("N,radii,seed", [(12, 36.0, None), (12, 38.0, None), (3, 35.0, 23), (12, 35.0, 23)])
def test_four_steppers_speculating(ctx, pkg, orc, N, radii, seed):
    rec, x0, r_max, c3, native = _problem(pkg, N, radii, seed)
    want, _, spec, _ = _loops(ctx, pkg, rec, x0, r_max, _kwargs(pkg, x0, r_max, c3, native), [], world=4)
    (x, stats), rounds = spec
    rule = _host_rule(pkg, orc, N, radii, seed)
    assert_matches_host_rule((x, stats), rule)
    had_I = radii > 30.0 * pc.TAN50
    assert [r for r in rounds if r] == ppc.rounds_written_out([(it[0], it[3] is not None) for it in rule["iters"]],
                                                              had_I, 4)
    assert max(rounds) >= 2
    if radii == 35.0:   # x0 is feasible; the first iteration is unsuccessful and leaves an I: it does not chain
        assert rule["iters"][0][0] == "unsuccessful" and rule["iters"][0][3] is not None and rounds[0] == 1


def test_entry_points_do_not_mix(ctx, pkg):
    lib = pkg._lib
    L = pkg.load_library()
    rec, x0, r_max, c3, native = _problem(pkg, 3, 36.0)
    ctx.set_points_records(rec)
    kw = _kwargs(pkg, x0, r_max, c3, native)
    prog = ctx.mads_prog_stepper(x0, r_max, 0.0, **kw)
    plain = ctx.mads_stepper(x0, r_max, 0.0, **{k: v for k, v in kw.items() if k not in ("prog", "h_max0")})
    try:
        done, bo, bi, part = ctypes.c_int32(), ctypes.c_double(), ctypes.c_int64(), lib.ProgPart()
        E = lib.MAC_E_INVAL
        assert L.mac_mads_poll(prog._h, ctypes.byref(done), ctypes.byref(bo), ctypes.byref(bi)) == E
        assert "prog stepper" in L.mac_last_error().decode()
        assert L.mac_mads_poll_ahead(prog._h, 0, ctypes.byref(done), ctypes.byref(bo), ctypes.byref(bi), None) == E
        assert L.mac_mads_update(prog._h, 0.0, -1) == E and L.mac_mads_advance(prog._h, 0.0, -1, None) == E
        assert L.mac_mads_poll_prog(plain._h, 0, ctypes.byref(done), ctypes.byref(part)) == E
        assert L.mac_mads_advance_prog(plain._h, ctypes.byref(part), None, None) == E
        assert L.mac_mads_result_prog(plain._h, None, None, None, None) == E
        # a record of another iteration is refused, and the stepper stays where it was
        _, p1 = prog.poll(1)
        assert p1.tag == 2
        with pytest.raises(lib.MaxCoverError, match="tag"):
            prog.advance(p1)
        _, p0 = prog.poll(0)
        assert p0.tag == 1 and prog.advance(p0)[0] in prog.OUTCOMES
        assert prog.result()[1]["iterations"] == 1
    finally:
        prog.close()
        plain.close()


def test_no_prog_launches_nothing_from_k_prog(ctx, pkg):
    """mac_mads_begin_prog without a prog (NULL, or n_cons = 0) is mac_mads_begin_mesh: a plain stepper,
    the plain loop's iterates, no launch of prog_h_kernel, prog_select_kernel or prog_part_kernel."""
    lib = pkg._lib
    L = pkg.load_library()
    rec, x0, r_max, c3, native = _problem(pkg, 12, 36.0)
    ctx.set_points_records(rec)
    base = ctx.mads_run(x0, r_max, 1e5, prev=c3.prev, d_lim=c3.d_lim, tan_half_fov=c3.tan_half_fov, **native)
    prm = lib.MadsParams(native["n_iter"], native["ell0"], native["ell_max"], native["seed"])
    ctx.profile(True)
    ctx.profile_read(reset=True)
    try:
        for pg in (None, lib.make_prog(dict(member=None, limit=None, n_cons=0))):
            h = ctypes.c_void_p()
            rc = L.mac_mads_begin_prog(ctx._h, lib._ptr(x0), x0.size, lib._ptr(r_max), 1e5, lib._ptr(c3.prev),
                                       lib._ptr(c3.d_lim), float(c3.tan_half_fov), ctypes.byref(prm), 0, 2 * x0.size,
                                       ctypes.byref(h), None, None, None, None,
                                       ctypes.byref(pg) if pg is not None else None)
            assert rc == 0 and h.value
            try:
                part, done = lib.ProgPart(), ctypes.c_int32()
                assert L.mac_mads_poll_prog(h, 0, ctypes.byref(done), ctypes.byref(part)) == lib.MAC_E_INVAL
                bo, bi = ctypes.c_double(), ctypes.c_int64()
                while True:
                    assert L.mac_mads_poll(h, ctypes.byref(done), ctypes.byref(bo), ctypes.byref(bi)) == 0
                    if done.value:
                        break
                    assert L.mac_mads_update(h, bo.value, bi.value) == 0
                out, st = np.empty_like(x0), lib.MadsStats()
                assert L.mac_mads_result(h, lib._ptr(out), ctypes.byref(st)) == 0
                assert out.tobytes() == base[0].tobytes() and st.f == base[1]["f"]
                assert st.iterations == base[1]["iterations"]
            finally:
                L.mac_mads_destroy(h)
        kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    finally:
        ctx.profile_read(reset=True)
        ctx.profile(False)
    assert "prog_h_kernel" not in kern and "prog_select_kernel" not in kern and kern


# ---------------------------------------------------------------- RCCL, a world of one

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def nccl1(ctx):
    import torch
    import torch.distributed as dist

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0,
                            world_size=1, device_id=dev)
    assert dist.get_backend() == "nccl"
    yield dev
    dist.destroy_process_group()


@pytest.mark.parametrize("gather", ["rccl", "torch"])
@pytest.mark.parametrize("loop", ["shard", "speculate"])
def test_prog_loops_over_rccl(nccl1, pkg, loop, gather):
    """dist.mads_prog_loop and dist.mads_prog_loop_speculative over RcclProgGather (the 96-byte record
    through mac_exchange_records) and over ProgGather on the nccl backend: Context.mads_run(prog=)'s result."""
    d = _dist(pkg)
    rec, x0, r_max, c3, native = _problem(pkg, 12, 38.0)
    kw = _kwargs(pkg, x0, r_max, c3, native)
    with pkg.Context(0) as c2:
        c2.set_points_records(rec)
        want = c2.mads_run(x0, r_max, 0.0, **kw)
        st = c2.mads_prog_stepper(x0, r_max, 0.0, **kw)
        try:
            g = d.RcclProgGather(c2, nccl1) if gather == "rccl" else d.ProgGather(nccl1)
            assert g.world == 1 and g.rank == 0
            if loop == "shard":
                got = d.mads_prog_loop(st, g)
            else:
                got = d.mads_prog_loop_speculative(st, g)
                # (one rank: one iteration per exchange, and the exchange that finds the loop done)
                assert got[1]["rounds"] == want[1]["iterations"] + 1
        finally:
            st.close()
    assert_same_native(got, want)
    assert got[1]["feasible_evaluations"] == want[1]["feasible_evaluations"]


# ---------------------------------------------------------------- Simulation

def test_simulation_with_a_shard_of_one_rank(ctx, pkg, firepoints):
    """Three MPC steps of Simulation(cons_prog=[create_cons1_progressive], penalty=0, shard=(0, 1)) equal the
    same simulation without a shard (tests/test_gpu_prog.py replays that one on the host)."""
    FS, TC = pkg.FullSimulation, pkg.TDM_Constraints
    N = 5
    x0 = np.round(pkg.Base_Functions.allocate_even_circles(15.0, N, 30.0, 255.0, 330.0))
    ctx.set_algo("auto")
    ctx.set_chain("auto")
    runs = []
    for shard in (None, (0, 1)):
        sim = FS.Simulation(ctx, x0, firepoints=firepoints, N_iter=30, seed=20250216,
                            cons_prog=[TC.create_cons1_progressive], penalty=0, shard=shard)
        runs.append(([sim.step() for _ in range(3)], sim.outputs))
    (ra, oa), (rb, ob) = runs
    keys = ("points", "f", "iterations", "evaluations", "h", "has_feasible", "dominating", "improving", "unsuccessful",
            "feasible_evaluations", "successes", "rejected_polls")
    for a, b, xa, xb in zip(ra, rb, oa, ob):
        assert xa.tobytes() == xb.tobytes()
        assert {k: a[k] for k in keys} == {k: b[k] for k in keys}
    assert any(r["dominating"] >= 1 and r["unsuccessful"] >= 1 for r in ra)
