"""CPU: the progressive barrier's shard-partial record (csrc/prog_rule.h, include/maxcover.h
mac_prog_part; DESIGN.md section 4 "Progressive barrier") and the host side of the prog stepper.

The record: tests/prog_cases.select_cases() (410 cases) split into 1, 2, 3 and 8 shards whose edges sit on
the wave and block sizes of prog_part_kernel (tests/prog_part_cases.py; one shard empty, the merge order
shuffled) must give select_written_out's ProgRec byte for byte: through prog_rule.h on the host compiler
(tests/host/prog_rule_check.cpp, plain and under the address and undefined-behaviour sanitizers: a
stand-alone program, nothing preloaded), through the Python mirrors TDM_STATIC_opt.prog_part / prog_merge /
prog_finish, and through the exported mac_prog_merge. f, h and g are selected, never summed: every
comparison is == on bits.

The stepper: TDM_STATIC_opt.ProgPollStepper under dist.mads_prog_loop and
dist.mads_prog_loop_speculative (one process, and two gloo ranks) against TDM_STATIC_opt.mads(cons_prog=) on
the oracle's objective; mac_mads_begin_prog's start errors with a NULL context."""
import ctypes
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import prog_cases as pc
import prog_part_cases as ppc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "maximumareacoverageoptimization.jl_amd", "csrc")


def _dist(pkg):
    from importlib import import_module
    return import_module(pkg.__name__ + ".dist")


# ---------------------------------------------------------------- the record

@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """The check program, plain and under the sanitizers (stand-alone programs: nothing preloaded)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the package's own build needs one)")
    d = tmp_path_factory.mktemp("prog_rule")
    src = os.path.join(ROOT, "tests", "host", "prog_rule_check.cpp")
    base = [cxx, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC]
    plain, san = str(d / "prog_rule_check"), str(d / "prog_rule_check_san")
    subprocess.run(base + ["-O1", "-o", plain, src], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", san, src], check=True)
    return plain, san


def _write_table(path):
    out, n = [], 0
    for case, want, splits in ppc.split_cases():
        K = case["K"]
        head = [struct.pack("<3q4d2q", K, case["has_F"], case["has_I"], case["F_f"], case["I_f"], case["I_h"],
                            case["h_max"], case["obj"][0] is not None, case["obj"][1] is not None)]
        for c in (0, 1):
            if case["obj"][c] is not None:
                head += [np.asarray(case["obj"][c], dtype="<f8").tobytes(), np.asarray(case["h"][c], dtype="<f8").tobytes()]
        head = b"".join(head)
        tail = pc.record_bytes(want) + struct.pack("<q", ppc.chains_written_out(want, bool(case["has_I"])))
        for shards in splits:
            out += [head, struct.pack("<q", len(shards)), b"".join(struct.pack("<2q", lo, hi) for lo, hi in shards), tail]
            n += 1
    with open(path, "wb") as fh:
        fh.write(struct.pack("<q", n) + b"".join(out))
    return n


def test_the_table_is_the_one_the_issue_names():
    sc = ppc.split_cases()
    assert len(sc) == 410 and {c["K"] for c, _, _ in sc} >= {1, 63, 64, 65, 255, 256, 257, 3072, 6600}
    # the hand-written cases carry their own answers, and the written-out rule agrees with them
    hand = [(c, w) for c, w, _ in sc if c["want"] is not None]
    assert len(hand) == 14
    for c, w in hand:
        got = pc.select_written_out(*pc.rule_args(c), c["obj"], c["h"], c["K"])
        assert pc.record_bytes(got) == pc.record_bytes(w), c["name"]
    # every split has an empty shard from two ranks on, and the shards partition the poll
    for c, _, splits in sc:
        assert [len(s) for s in splits] == list(ppc.WORLDS)
        for s in splits:
            assert sorted(s)[0][0] == 0 and max(hi for _, hi in s) == c["K"]
            assert len(s) == 1 or any(lo == hi for lo, hi in s)
    # unsuccessful iterations that change I (no I before, an infeasible candidate evaluated): what ends
    # a speculative round early
    n = sum((w[0] & 255) == 2 and not ppc.chains_written_out(w, bool(c["has_I"])) for c, w, _ in sc)
    assert n == 37 and all(not c["has_I"] and w[5] >= 0 for c, w, _ in sc
                           if (w[0] & 255) == 2 and not ppc.chains_written_out(w, bool(c["has_I"])))


def test_rule_header_on_the_host_compiler(checkers, tmp_path):
    path = str(tmp_path / "table.bin")
    n = _write_table(path)
    assert n == 410 * 4
    for exe in checkers:
        r = subprocess.run([exe, path], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"cases {n} " in r.stdout and r.stdout.rstrip().endswith(": ok")


@pytest.fixture(scope="module")
def mirror_parts(pkg):
    """Per case and split: the shard records of the Python mirror (computed once, shared below)."""
    TS = pkg.TDM_STATIC_opt
    out = []
    for q, (case, want, splits) in enumerate(ppc.split_cases()):
        args = pc.rule_args(case)
        out.append([[TS.prog_part(*args, ppc.shard_cands(case, lo, hi), q + 1) for lo, hi in shards]
                    for shards in splits])
    return out


def test_python_mirrors(pkg, mirror_parts):
    TS = pkg.TDM_STATIC_opt
    assert TS.prog_part_empty() == (0, 0, math.inf, -1, 0, -1.0, math.inf, math.inf, -1, math.inf, math.inf, -1)
    for (case, want, splits), per_split in zip(ppc.split_cases(), mirror_parts):
        args = pc.rule_args(case)
        for parts in per_split:
            merged = TS.prog_merge(parts)
            assert ppc.part_bytes(TS.prog_merge(parts[::-1])) == ppc.part_bytes(merged), case["name"]
            rec = TS.prog_finish(merged, *args)
            assert pc.record_bytes(rec) == pc.record_bytes(want), (case["name"], len(parts), rec, want)
            assert TS.prog_chains(rec, bool(case["has_I"])) == ppc.chains_written_out(want, bool(case["has_I"]))
    with pytest.raises(ValueError, match="tags"):
        TS.prog_merge([TS.prog_part_empty(1), TS.prog_part_empty(2)])


def test_exported_merge_needs_no_context(pkg, mirror_parts):
    lib, TS = pkg._lib, pkg.TDM_STATIC_opt
    assert ctypes.sizeof(lib.ProgPart) == 96 and lib.ProgPart.drop_g.offset == 88 and lib.ProgPart.h_below.offset == 40
    assert {"mac_mads_begin_prog", "mac_mads_poll_prog", "mac_prog_merge", "mac_mads_advance_prog",
            "mac_mads_result_prog"} <= set(lib.EXPORTS)
    for (case, want, _), per_split in zip(ppc.split_cases(), mirror_parts):
        for parts in per_split:
            got = lib.prog_merge([lib.ProgPart(*p) for p in parts])
            assert bytes(got) == ppc.part_bytes(TS.prog_merge(parts)), case["name"]
            assert pc.record_bytes(TS.prog_finish(got.as_tuple(), *pc.rule_args(case))) == pc.record_bytes(want)
    # the words a gather exchanges carry the record bit for bit (NaN-patterned index words included)
    odd = lib.ProgPart(5, 1, math.nan, -1, 1, -1.0, -0.0, 5e-324, 0x7FF0000000000001, math.inf, math.inf, -1)
    assert bytes(lib.ProgPart.from_words(odd.words())) == bytes(odd)
    # unequal tags, no record, null arguments
    L = pkg.load_library()
    with pytest.raises(lib.MaxCoverError) as e:
        lib.prog_merge([lib.ProgPart(*TS.prog_part_empty(3)), lib.ProgPart(*TS.prog_part_empty(4))])
    assert e.value.code == lib.MAC_E_INVAL and "tags" in str(e.value)
    one = lib.ProgPart(*TS.prog_part_empty(1))
    assert L.mac_prog_merge(ctypes.byref(one), 0, ctypes.byref(one)) == lib.MAC_E_INVAL
    assert L.mac_prog_merge(None, 1, ctypes.byref(one)) == lib.MAC_E_INVAL
    assert L.mac_prog_merge(ctypes.byref(one), 1, None) == lib.MAC_E_INVAL


# ---------------------------------------------------------------- the stepper's host mirror

# (N, radii, seed). Radii 35.0: x0 is feasible and h_max starts at +inf, so trial points that raise a
# radius are infeasible and evaluated. Seed 23 (found by scanning seeds 0..399 on the CPU, for N = 3 and
# N = 12 alike): no feasible trial point of the first poll improves F, so the first iteration is
# unsuccessful and I appears on it: an unsuccessful iteration that does not chain.
RUNS = [(3, 36.0, 99), (3, 38.0, 99), (3, 35.0, 23), (12, 36.0, 99), (12, 38.0, 99), (12, 35.0, 23)]
_runs = {}


def _problem(pkg, orc, N, radii):
    """(x0, obj, cons_ext, cons_prog): the oracle's objective with penalty 0, memoised per point (every
    form of the loop evaluates the same points)."""
    key = ("problem", N, radii)
    if key not in _runs:
        TC = pkg.TDM_Constraints
        rec, x0, r_max = pc.recipe(pkg, N, 7, 320, 40, radii)
        seen = {}

        def obj(v):
            k = np.asarray(v, dtype=np.float64).tobytes()
            if k not in seen:
                seen[k] = orc.ref_objective(v, rec, r_max, 0.0)
            return seen[k]

        c3 = TC.create_cons3(x0, pc.FOV, np.full(N, 10.0))
        _runs[key] = x0, obj, [TC.cons1, c3], [TC.create_cons1_progressive(r_max)]
    return _runs[key]


def _kw(seed):
    return dict(pc.KW, seed=seed)


def _reference(pkg, orc, N, radii, seed):
    key = ("ref", N, radii, seed)
    if key not in _runs:
        x0, obj, cons, progs = _problem(pkg, orc, N, radii)
        _runs[key] = pkg.TDM_STATIC_opt.mads(x0, obj, cons, cons_prog=progs, **_kw(seed))
    return _runs[key]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def assert_same_run(res, ref):
    """history, F, I, h_max and the counts, exactly."""
    assert len(res.history) == len(ref.history)
    for got, want in zip(res.history, ref.history):
        assert got[0] == want[0] and got[7] == want[7]
        assert _same(got[1], want[1]) and got[2] == want[2]
        assert _same(got[3], want[3]) and got[4] == want[4] and got[5] == want[5]
        assert got[6] == want[6]
    assert _same(res.x, ref.x) and res.x_cost == ref.x_cost
    assert _same(res.i, ref.i) and res.i_cost == ref.i_cost and res.i_h == ref.i_h
    assert res.h_max == ref.h_max
    a, b = res.status, ref.status
    for k in ("iteration", "function_evaluations", "dominating", "improving", "unsuccessful", "successes",
              "two_centre_polls", "evaluated", "optimization_status"):
        assert getattr(a, k) == getattr(b, k), k


def _sharded(pkg, orc, N, radii, seed, shards):
    """mads_prog_loop over one stepper per shard, in lock step (prog_part_cases.lock_step)."""
    TS = pkg.TDM_STATIC_opt
    x0, obj, cons, progs = _problem(pkg, orc, N, radii)
    st = [TS.ProgPollStepper(x0, obj, cons, progs, shard=sh, **_kw(seed)) for sh in shards]
    res, _ = ppc.lock_step(st, _dist(pkg).mads_prog_loop)
    for s in st[1:]:
        assert_same_run(s.result(), res)
    return res


def _speculative(pkg, orc, N, radii, seed, world):
    TS = pkg.TDM_STATIC_opt
    x0, obj, cons, progs = _problem(pkg, orc, N, radii)
    st = [TS.ProgPollStepper(x0, obj, cons, progs, **_kw(seed)) for _ in range(world)]
    return ppc.lock_step(st, _dist(pkg).mads_prog_loop_speculative, ahead=True)


@pytest.mark.parametrize("N,radii,seed", RUNS)
def test_host_stepper_matches_mads_cons_prog(pkg, orc, N, radii, seed):
    ref = _reference(pkg, orc, N, radii, seed)
    K = 6 * N
    assert_same_run(_sharded(pkg, orc, N, radii, seed, [None]), ref)                       # the whole poll
    assert_same_run(_sharded(pkg, orc, N, radii, seed, [(0, K // 2), (K // 2, K)]), ref)   # two shards
    assert_same_run(_sharded(pkg, orc, N, radii, seed, [(0, 5), (5, 5), (5, K)]), ref)     # one of three empty
    res, rounds = _speculative(pkg, orc, N, radii, seed, 4)
    assert_same_run(res, ref)
    assert res.status.rounds == len(rounds) and sum(rounds) == ref.status.iteration
    assert all(0 <= r <= 4 for r in rounds)
    # an exchange applies iterations up to the first that does not chain: from the reference's history
    want = ppc.rounds_written_out([(h[0], h[3] is not None) for h in ref.history], radii > 30.0 * pc.TAN50, 4)
    assert [r for r in rounds if r] == want


def test_the_reference_runs_have_every_feature(pkg, orc):
    """On TDM_STATIC_opt.mads(cons_prog=)'s own histories, so that no comparison above passes trivially."""
    seen = set()
    for N, radii, seed in RUNS:
        ref = _reference(pkg, orc, N, radii, seed)
        s = ref.status
        assert s.dominating >= 1 and s.improving >= 1 and s.unsuccessful >= 1, (N, radii)
        seen |= {"two"} if s.two_centre_polls >= 1 else set()
        outs = [h[0] for h in ref.history]
        if radii == 35.0:
            # x0 is feasible (h = 0, no I); the first iteration is unsuccessful and leaves an I
            assert ref.history[0][0] == "unsuccessful" and ref.history[0][3] is not None
            assert ref.history[0][7] == 1 and ref.history[1][7] == 2
            seen.add("I appears on an unsuccessful iteration")
        # two unsuccessful iterations in a row with I unchanged: a speculative round applies both
        for a, b in zip(ref.history, ref.history[1:]):
            if a[0] == b[0] == "unsuccessful" and _same(a[3], b[3]) and a[3] is not None:
                seen.add((N, radii, "chain"))
        assert (N, radii, "chain") in seen, outs
    assert {"two", "I appears on an unsuccessful iteration"} <= seen


def test_speculative_rounds_apply_more_than_one_iteration(pkg, orc):
    for N, radii, seed in RUNS:
        res, rounds = _speculative(pkg, orc, N, radii, seed, 4)
        assert max(rounds) >= 2 and len([r for r in rounds if r]) < res.status.iteration, (N, radii, rounds)
        if radii == 35.0:   # the first iteration is unsuccessful and does not chain: a round of one
            assert rounds[0] == 1


# ---------------------------------------------------------------- gloo, world 2

def _gloo_rank(rank, world, port, root, out_dir):
    import sys
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch.distributed as tdist
    import __graft_entry__ as ge
    import prog_cases as pc_
    pkg = ge.load_package()
    orc = ge.load_oracle()
    tdist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from importlib import import_module
        TS, TC, dist = pkg.TDM_STATIC_opt, pkg.TDM_Constraints, import_module(pkg.__name__ + ".dist")
        N, radii, seed = 3, 35.0, 23
        rec, x0, r_max = pc_.recipe(pkg, N, 7, 320, 40, radii)
        obj = lambda v: orc.ref_objective(v, rec, r_max, 0.0)   # noqa: E731
        cons = [TC.cons1, TC.create_cons3(x0, pc_.FOV, np.full(N, 10.0))]
        progs = [TC.create_cons1_progressive(r_max)]
        kw = dict(pc_.KW, seed=seed)
        gather = dist.ProgGather("cpu")
        K = 6 * N
        sh = dist.shard_range(K, rank, world)
        a = dist.mads_prog_loop(TS.ProgPollStepper(x0, obj, cons, progs, shard=sh, **kw), gather)
        b = dist.mads_prog_loop_speculative(TS.ProgPollStepper(x0, obj, cons, progs, **kw), gather)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"),
                 **{f"{n}_{k}": v for n, r in (("a", a), ("b", b)) for k, v in dict(
                     x=np.full(3 * N, np.nan) if r.x is None else r.x, i=np.full(3 * N, np.nan) if r.i is None else r.i,
                     nums=np.array([r.x_cost, r.i_cost, r.h_max, r.status.iteration, r.status.dominating,
                                    r.status.improving, r.status.unsuccessful, r.status.evaluated,
                                    r.status.two_centre_polls, r.status.function_evaluations]),
                     outs=np.array([("dominating", "improving", "unsuccessful").index(h[0]) for h in r.history]),
                     rounds=np.array([getattr(r.status, "rounds", -1)])).items()})
    finally:
        tdist.destroy_process_group()


def test_gloo_world_2_ends_on_the_sequential_run(pkg, orc, tmp_path):
    import socket
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_gloo_rank, args=(2, port, ROOT, str(tmp_path)), nprocs=2, join=True)
    ref = _reference(pkg, orc, 3, 35.0, 23)
    s = ref.status
    nums = np.array([ref.x_cost, ref.i_cost, ref.h_max, s.iteration, s.dominating, s.improving, s.unsuccessful,
                     s.evaluated, s.two_centre_polls, s.function_evaluations])
    outs = np.array([("dominating", "improving", "unsuccessful").index(h[0]) for h in ref.history])
    for rank in (0, 1):
        with np.load(str(tmp_path / f"rank{rank}.npz")) as z:
            for loop in ("a", "b"):
                assert z[f"{loop}_x"].tobytes() == ref.x.tobytes() and z[f"{loop}_i"].tobytes() == ref.i.tobytes()
                assert z[f"{loop}_nums"].tobytes() == nums.tobytes(), (rank, loop, z[f"{loop}_nums"], nums)
                assert np.array_equal(z[f"{loop}_outs"], outs)
            assert z["a_rounds"][0] == -1 and 0 < z["b_rounds"][0] < s.iteration


# ---------------------------------------------------------------- mac_mads_begin_prog's start errors

def _prog(lib, member, limit, n_cons, reserved=0, h_max0=-1.0):
    p = lib.make_prog(dict(member=member, limit=limit, n_cons=n_cons, h_max0=h_max0))
    p.reserved = reserved
    return p


def _begin_call(pkg, x0, prog):
    lib = pkg._lib
    L = pkg.load_library()
    x = np.asarray(x0, dtype=np.float64)
    N = x.size // 3
    rm = np.full(N, 35.0)
    prm = lib.MadsParams(5, 2, 5, 99)
    h = ctypes.c_void_p(0xDEAD)
    rc = L.mac_mads_begin_prog(None, lib._ptr(x), x.size, lib._ptr(rm), 0.0, None, None, 1.0, ctypes.byref(prm), 0,
                               2 * x.size, ctypes.byref(h), None, None, None, None,
                               ctypes.byref(prog) if prog is not None else None)
    assert h.value is None   # *out is cleared
    return rc, L.mac_last_error().decode()


def test_begin_prog_start_errors_before_the_context(pkg):
    lib = pkg._lib
    ones, lim = np.ones(3, dtype=np.uint32), np.full(3, 35.0)
    x0 = np.array([1.0, 2, 3, 4, 5, 6, 36.0, 36.0, 34.0])
    bad = [
        _prog(lib, ones, lim, -1), _prog(lib, ones, lim, 33),          # n_cons outside [0, 32]
        _prog(lib, None, lim, 1), _prog(lib, ones, None, 1),           # n_cons > 0 with a null array
        _prog(lib, np.array([1, 2, 1], dtype=np.uint32), lim, 1),      # a bit at or above n_cons
        _prog(lib, np.array([1, 1, 1 << 31], dtype=np.uint32), lim, 31),
        _prog(lib, ones, lim, 1, reserved=1),                          # reserved
        _prog(lib, ones, np.array([35.0, math.nan, 35.0]), 1),         # a NaN limit
    ]
    for p in bad:
        rc, msg = _begin_call(pkg, x0, p)
        assert rc == lib.MAC_E_INVAL and "mac_prog" in msg, msg
    big = _prog(lib, np.ones(2049, dtype=np.uint32), np.zeros(2049), 1)
    rc, msg = _begin_call(pkg, np.zeros(3 * 2049), big)
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "2048" in msg
    nan0 = x0.copy()
    nan0[6] = math.nan
    rc, msg = _begin_call(pkg, nan0, _prog(lib, ones, lim, 1))
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "NaN" in msg
    # h(x0) = (1 + 1)^2 = 4 > h_max0 = 3.5
    rc, msg = _begin_call(pkg, x0, _prog(lib, ones, lim, 1, h_max0=3.5))
    assert rc == lib.MAC_E_INVAL and "mac_prog" in msg and "h_max0" in msg
    # a start the barrier admits, and a call without a prog (mac_mads_begin_mesh itself), get as far as the
    # context check
    for p in (_prog(lib, ones, lim, 1, h_max0=4.0), _prog(lib, ones, lim, 1), _prog(lib, None, None, 0), None):
        rc, msg = _begin_call(pkg, x0, p)
        assert rc == lib.MAC_E_INVAL and "mac_prog" not in msg and "context" in msg, msg
    # the step calls refuse a null stepper
    L = pkg.load_library()
    part, done = lib.ProgPart(), ctypes.c_int32()
    assert L.mac_mads_poll_prog(None, 0, ctypes.byref(done), ctypes.byref(part)) == lib.MAC_E_INVAL
    assert L.mac_mads_advance_prog(None, ctypes.byref(part), None, None) == lib.MAC_E_INVAL
    assert L.mac_mads_result_prog(None, None, None, None, None) == lib.MAC_E_INVAL


def test_python_surface(pkg):
    x0 = np.array([1.0, 2, 3, 4, 5, 6, 36.0, 36.0, 34.0])
    prog = dict(member=np.ones(3, dtype=np.uint32), limit=np.full(3, 35.0), n_cons=1)
    with pytest.raises(ValueError, match="mads_prog_stepper"):   # the plain stepper points to the prog one
        pkg.Context.mads_stepper(None, x0, np.full(3, 35.0), prog=prog)
    with pytest.raises(ValueError, match="prog"):                 # ... which needs a constraint
        pkg.Context.mads_prog_stepper(None, x0, np.full(3, 35.0), prog=None)
    with pytest.raises(ValueError, match="member and limit"):
        pkg.Context.mads_prog_stepper(None, x0, np.full(3, 35.0),
                                      prog=dict(member=np.ones(2, dtype=np.uint32), limit=np.zeros(2), n_cons=1))
