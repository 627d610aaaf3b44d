"""The native MADS driver on lists whose weights differ (tests/test_weighted_mads_cases.py checks the
cases on the CPU, tests/test_gpu_mads_weighted.py runs the device over them).

csrc/eval_plan.h sets `counts = poll_possible && w_uniform`: equal weights take the integer count rows
of the poll chains, anything else their fp64 credit rows, and csrc/kernel_select.h turns the bit into
builds of their own (fiw_kernel<kCounts, kMat, kMesh>, fin2_kernel<kCounts, kMat, kXY, kMesh>,
shared_bits_kernel in place of shared_or_kernel, the fp64 rows of coverage_poll_kernel and
finalize_kernel<kXY, kMesh>). Every other test of the driver runs on equal weights; the cases here are
the driver's recipes (test_gpu_poll_vars._recipe) on two lists that are not:

  "weighted"   the 160 x 160 lattice with weights 0.25 (1 + floor(31 u)), u from SplitMix64(4711):
               31 distinct weights, 0.25 .. 7.75, summing to 102,449.25
  "regions"    the equal-weight lattice (25.0) with the entries strictly inside REGION_BOXES at 100.0:
               what Context.set_regions(*REGION_BOXES, w_high=100.0) makes of it on the device; here
               test_gpu_regions.ref_override on the records

Every partial sum of either list is a multiple of 0.25 far below 2^53: exact in any order, so every
comparison is == / array_equal.

Reference side: test_gpu_poll_vars._reference (TDM_STATIC_opt.mads over orc.ref_objective, one trial
point at a time, cons1 / cons3 and any swarm or motion constraint as host callables; for the
progressive barrier test_gpu_prog's host rule, TDM_STATIC_opt.mads(cons_prog=)), each run under a cache
key of its own in that module's table; libmaxcover is not on that side. `conditions` asserts of every
reference run that it is no trivial one (successes > 3, f < f0) and that its final iterate is not the
equal-weight run's of the same recipe: a kernel that ignored the weights, or read w[0], cannot pass.

numpy, the oracle and the package's host code only; deterministic; nothing read from outside the
repository."""
import ctypes
import math

import numpy as np

import prog_cases as pc
import shape_edges as se
import test_gpu_poll_vars as tpv
import test_gpu_prog as tp
import test_gpu_regions as tr
from test_gpu_mads_motion import host_constraints, motion_for

W_HI = 100.0
# (x_LB, x_UB, y_LB, y_UB): one box over part of the clustered layout's square, one wide band above it
REGION_BOXES = ([340.0, 100.0], [440.0, 700.0], [300.0, 440.0], [420.0, 700.0])
D_SEP = 5.0        # x0's closest pair in the spread N = 12 layout is exactly 5.0 apart
PROG_RADII = 38.0  # above r_max = 35.75: the start is infeasible, both centres are polled

# name: N, the layout's (lo, span), the polled variables, the mesh (None: the unit mesh), constraints
CASES = {
    "full": dict(N=12, lo=320, span=160, pv="xyr", gran=None),
    "clustered": dict(N=12, lo=380, span=40, pv="xyr", gran=None),
    # (18 disks in the same square: more than kBitsMinDisks = 16 have neighbours, so the five-launch
    # chain launches the shared-entry pass of its own accord)
    "crowded18": dict(N=18, lo=380, span=40, pv="xyr", gran=None),
    "xy18": dict(N=18, lo=320, span=160, pv="xy", gran=None),
    "xy17": dict(N=17, lo=320, span=160, pv="xy", gran=None),
    "mesh": dict(N=12, lo=320, span=160, pv="xyr", gran=(1.0, 0.125)),
    "mesh01": dict(N=12, lo=320, span=160, pv="xyr", gran=(1.0, 0.1)),
    "xy16": dict(N=16, lo=380, span=40, pv="xy", gran=(0.5, 0.125)),
    # entries on the disks' boundaries (BAND_R below): xy polls, so the radii stay there
    "band18": dict(N=18, lo=320, span=160, pv="xy", gran=None, radii="band"),
    "band18m": dict(N=18, lo=320, span=160, pv="xy", gran=(0.5, 0.125), radii="band"),
    "cons8": dict(N=12, lo=320, span=160, pv="xyr", gran=None, extra="cons8"),
    "motion": dict(N=12, lo=320, span=160, pv="xyr", gran=None, extra="motion"),
}
# the recipes of the issue's table: (successes, function evaluations) of the weighted reference run
TABLE = {"full": (15, 869), "xy18": (15, 245), "clustered": (15, 992), "mesh": (16, 433), "xy16": (16, 383)}
REGION_CASES = ("full", "mesh", "xy16", "band18", "band18m")
# A lattice entry lies (2 i + 1) / 2 from an integer centre per axis, so its squared distance is some
# n + 1/2 and no integer or eighth radius comes within 1 / 64 of it: the fp32 filter's band around the
# threshold, and with it fiw_kernel's per-entry fp64 credit, is not entered on integer centres. With
# R = sqrt(1300.5) (4 R^2 = 5202 = 51^2 + 51^2 = 21^2 + 69^2) a disk whose integer centre is 2 or 3
# mod 5 in x and y has entries at (+-25.5, +-25.5), (+-10.5, +-34.5) or (+-34.5, +-10.5) from it:
# within an ulp of the threshold, decided in fp64 (covered or not is the oracle's to say).
BAND_R = math.sqrt(1300.5)

_LISTS = {}


def weights(pkg):
    u = pkg.workloads.SplitMix64(4711).uniform(25600)
    return 0.25 * (1.0 + np.floor(u * 31.0))


def records(pkg, lst="weighted"):
    """The records of a list ("weighted", "regions", or "equal": the lattice as it is), read-only."""
    if lst not in _LISTS:
        rec = tpv._grid(pkg)
        if lst == "weighted":
            w = weights(pkg)
            rec = np.stack([rec[:, 0], rec[:, 1], w, w, np.zeros_like(w)], axis=1)
        elif lst == "regions":
            rec = tr.ref_override(rec, REGION_BOXES, W_HI)
        else:
            assert lst == "equal"
        rec.setflags(write=False)
        _LISTS[lst] = rec
    return _LISTS[lst]


def start(pkg, name):
    """(x0, r_max) of a case."""
    c = CASES[name]
    radii = BAND_R if c.get("radii") == "band" else 36.0
    _, x0, r_max = tpv._recipe(pkg, c["N"], 2024, c["lo"], c["span"], radii=radii)
    return x0, r_max


def boundary_entries(pkg, v):
    """The (disk, entry) pairs of circles v whose squared distance is within 1e-6 of the squared radius."""
    rec = records(pkg, "equal")
    N = v.size // 3
    n = 0
    for i in range(N):
        dx, dy = rec[:, 0] - v[i], rec[:, 1] - v[N + i]
        n += int(np.count_nonzero(np.abs(dx * dx + dy * dy - v[2 * N + i] * v[2 * N + i]) < 1e-6))
    return n


def mads_kw(name):
    """TDM_STATIC_opt.mads's keywords of a case, and the native driver's."""
    c = CASES[name]
    host = dict(tpv.MADS)
    native = dict(tpv.NATIVE, poll_vars=c["pv"])
    if c["gran"] is not None:
        host["granularity"] = c["gran"]
        native["granularity"] = c["gran"]
    return host, native


def candidates(name):
    c = CASES[name]
    return (4 if c["pv"] == "xy" else 6) * c["N"]


def _counted(c, into, q):
    def f(v):
        ok = bool(c(v))
        into[q] += not ok
        return ok
    return f


def motion(pkg, name):
    return motion_for(pkg, start(pkg, name)[0], 3)


def reference(pkg, orc, name, lst="weighted"):
    """The reference run of a case on a list (once per (list, case)): test_gpu_poll_vars._reference's
    record, with `rejected` (per host constraint of the case) added."""
    key = ("weighted_mads_cases", lst, name)
    c = CASES[name]
    x0, r_max = start(pkg, name)
    fresh = key not in tpv._REF
    rejected, extra = [], []
    if fresh and c.get("extra") == "cons8":
        rejected = [0]
        extra = [_counted(pkg.TDM_Constraints.create_cons8(D_SEP), rejected, 0)]
    if fresh and c.get("extra") == "motion":
        rejected = [0, 0, 0]
        extra = [_counted(h, rejected, q) for q, h in enumerate(host_constraints(pkg, motion(pkg, name)))]
    ref = tpv._reference(pkg, orc, key, records(pkg, lst), x0, r_max, swarm=extra, mads_kw=mads_kw(name)[0],
                         poll_vars=c["pv"])
    if fresh:
        ref["rejected"] = list(rejected)
    return ref


def conditions(pkg, orc, name, lst="weighted"):
    """Asserts that the reference run of (list, case) is no trivial one and that its iterate is not the
    equal-weight run's; returns it."""
    ref = reference(pkg, orc, name, lst)
    eq = reference(pkg, orc, name, "equal")
    assert ref["polled"] == tpv.MADS["N_iter"] * candidates(name), (name, ref["polled"])
    assert ref["succ"] > 3 and ref["f"] < ref["f0"], (name, lst, ref["succ"], ref["f"], ref["f0"])
    assert not np.array_equal(ref["x"], eq["x"]), (name, lst)
    if CASES[name].get("extra"):
        assert all(0 < r < ref["polled"] for r in ref["rejected"]), (name, ref["rejected"])
    return ref


def override_fraction(pkg):
    return float(np.mean(records(pkg, "regions")[:, 3] == W_HI))


def check(got, ref, x0, name):
    """What the driver tests check, exactly: test_gpu_poll_vars._check (for a full poll without its
    line on the radii, which only an xy poll holds)."""
    if CASES[name]["pv"] == "xy":
        return tpv._check(got, ref, x0)
    xn, st = got
    assert np.array_equal(xn, ref["x"])
    assert st["f"] == ref["f"]
    assert st["iterations"] == ref["it"]
    assert (st["status"] == 0) == ref["limit"]
    assert st["evaluations"] == 1 + ref["polled"]
    assert st["feasible_evaluations"] == ref["evals"] - 1
    assert st["successes"] == ref["succ"]
    assert st["slot_fallbacks"] == 0


# ---------------------------------------------------------------- the progressive barrier

# (seed 202 of 99 .. 599 searched on the CPU: at radii 38 most runs never find a feasible point in 30
# iterations, so never poll two centres; this one does, and its feasible incumbent is below f(x0))
PROG_KW = dict(pc.KW, seed=202)
PROG_NATIVE = dict(n_iter=PROG_KW["N_iter"], ell0=PROG_KW["ell0"], ell_max=PROG_KW["ell_max"], seed=PROG_KW["seed"])


def prog_reference(pkg, orc, lst="weighted"):
    """test_gpu_prog._reference's run (N = 12, penalty 0, create_cons1_progressive over every UAV, cons3;
    TDM_STATIC_opt.mads(cons_prog=) over the oracle's objective) on a list of this module, under a key of
    its own in that module's table: (res, rec, x0, r_max, c3)."""
    key = ("weighted_mads_cases", lst, "prog")
    if key not in tp._REF:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        rec = records(pkg, lst)
        _, x0, r_max = pc.recipe(pkg, 12, 2024, 320, 160, PROG_RADII)
        c3 = TC.create_cons3(x0, pc.FOV, np.full(12, 10.0))
        res = TS.mads(x0, lambda v: orc.ref_objective(v, rec, r_max, 0.0), [c3],
                      cons_prog=tp._progs(pkg, 12, r_max, False), granularity=None, poll_vars="xyr", h_max0=None,
                      **PROG_KW)
        tp._REF[key] = res, rec, x0, r_max, c3
    return tp._REF[key]


def prog_conditions(pkg, orc):
    """The barrier's run on the weighted list: both centres polled, more than three successes (dominating
    iterations), a feasible incumbent below f(x0), and a final iterate that is not the equal-weight
    run's. Returns prog_reference's tuple."""
    ref = prog_reference(pkg, orc)
    res, rec, x0, r_max, _ = ref
    eq = prog_reference(pkg, orc, "equal")[0]
    s = res.status
    assert s.two_centre_polls > 0 and s.successes == s.dominating > 3, vars(s)
    assert res.x is not None and res.x_cost < orc.ref_objective(x0, rec, r_max, 0.0), res.x_cost
    want, want_eq = (r.x if r.x is not None else r.i for r in (res, eq))
    assert not np.array_equal(want, want_eq)
    return ref


# ---------------------------------------------------------------- end to end

# Simulation(high_interest=True) takes the module's boxes, which lie outside the default 500 x 500
# DynamicArea, and its default w_high = (30 tan 50 deg)^2 pi is no multiple of 0.25: the case names a box
# that cuts the ignition block and w_high = 100, so that the list holds both weights and every sum is exact.
SIM_N = 16
SIM_BOXES = ([200.0], [262.0], [300.0], [349.0])
SIM_KW = dict(N_iter=10, seed=77)
SIM_MESH = (1.0, 0.125)
SIM_STEPS = 3
_SIM = {}


def sim_start(pkg, orc):
    """16 UAVs on a ring of radius 70 around the ignition block, radii at r_max but for two UAVs one
    mesh step (0.125) below it: step 1 polls every variable, and once those two radii are back the
    auto rule holds the radii (xy polls, K = 64: the smallest that takes the poll chains)."""
    tan = math.tan(pkg.FullSimulation.FOV / 2)
    ring = orc.ref_allocate_even_circles(70.0, SIM_N, 10 * tan, 250.0, 345.0)
    R = np.full(SIM_N, 30.0 * tan)
    R[:2] -= SIM_MESH[1]
    return np.concatenate([np.round(ring[:2 * SIM_N]), R])


class HostArea:
    """What test_gpu_regions._replay reads of a DynamicArea, for the default area, without a device:
    grid_size, ignition and initial_points (csrc/fire.hip mac_fire_initial_points: y outer, x inner)."""
    grid_size = (100, 100)
    ignition = (40, 60, 69, 71)

    def initial_points(self):
        ix0, ix1, iy0, iy1 = self.ignition
        return np.array([[xx * 5.0 - 2.5, yy * 5.0 - 2.5, 25.0, 25.0, 0.0]
                         for yy in range(iy0, iy1 + 1) for xx in range(ix0, ix1 + 1)])


def sim_replay(pkg, orc, D=None):
    """test_gpu_regions._replay of the case (once), with its conditions asserted: a step that polls
    every variable, a step on the xy poll, both weights in the list at every MADS run, every run moved."""
    if "replay" not in _SIM:
        x0 = sim_start(pkg, orc)
        want = tr._replay(pkg, orc, D if D is not None else HostArea(), x0, SIM_BOXES, W_HI, SIM_STEPS,
                          SIM_KW["N_iter"], SIM_KW["seed"], poll_vars="auto", granularity=SIM_MESH)
        pvs = [r["poll_vars"] for r in want]
        assert "xy" in pvs and "xyr" in pvs, pvs
        for r in want:
            assert set(np.unique(r["lst"][:, 3])) == {25.0, W_HI}, r["t"]
            assert not np.array_equal(r["x"], r["input"]), r["t"]
            assert 2 * (2 if r["poll_vars"] == "xy" else 3) * SIM_N >= se.kPollMinK
        _SIM["replay"] = x0, want
    return _SIM["replay"]


# ---------------------------------------------------------------- the plan

def route(pkg, N, pv, gran, chain, keys):
    """eval_plan's words for the driver's generated poll of N disks (pv: the polled variables, gran: the
    mesh or None) on a list with w_uniform = 0, as a dict of shape_edges.PLAN_FIELDS. Through
    mac_diag_route_keys (mac_diag_route with the key mode); shape_edges.plan is the same call without a
    key mode and is compared wherever it applies (no mesh, or value keys)."""
    n_p = (2 if pv == "xy" else 3) * N
    K = 2 * n_p
    np_ = n_p if pv == "xy" else 0
    g = np.zeros(0) if gran is None else np.ascontiguousarray(pkg._lib.mesh_granularity(gran, 3 * N)[:n_p])
    lib, L = pkg._lib, pkg.load_library()
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.mac_diag_route_keys.argtypes = [i64p, ctypes.c_double, i64p, ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                                      ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.mac_diag_route_keys.restype = ctypes.c_int32
    M = 160 * 160
    # (algo, chain, cus, M, w_uniform, kind, np, k0, mesh, mst, route_five, b, want_area, want_obj, cons3,
    # mask, tiled, N, K, key mode): the pipelined loop's poll (mst) with cons3
    args = (lib.ALGOS["auto"], lib.CHAINS[chain], 256, M, 0, se.SRC_GENERATED, np_, 0, 0, True, 0, 4,
            False, True, True, False, True, N, K, 1 if keys else 0)
    out = (ctypes.c_int64 * len(se.PLAN_FIELDS))()
    five = ctypes.c_int32(-1)
    rc = L.mac_diag_route_keys((ctypes.c_int64 * len(args))(*(int(a) for a in args)), 0.0, out, len(out),
                               g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if g.size else None, g.size, 0,
                               ctypes.byref(five))
    assert rc == 0, (rc, N, pv, gran)
    p = dict(zip(se.PLAN_FIELDS, (int(v) for v in out)))
    if not (keys and g.size):
        q = se.plan(N, K, chain=chain, kind=se.SRC_GENERATED, np_=np_, mesh=bool(g.size), mst=True, b=4,
                    cons3=True, M=M, w_uniform=False, route_five=bool(five.value))
        assert vars(q) == p, (N, pv, gran, chain, vars(q), p)
    return p


def assert_route(pkg, name, chain, keys=False, N=None, fused=None):
    """The plan of a case (at another N where given) under a forced chain: fp64 credit rows, the intended
    kMesh build, and the fused chain where it is forced (fused: another expectation, for a K past the
    fused chain's limit)."""
    c = CASES[name]
    p = route(pkg, c["N"] if N is None else N, c["pv"], c["gran"], chain, keys)
    want_mesh = 0 if c["gran"] is None else 2 if keys else 1
    assert p["poll_possible"] == 1 and p["counts"] == 0 and p["mesh"] == want_mesh, (name, chain, keys, p)
    assert p["fused_eligible"] == ((1 if chain == "fused" else 0) if fused is None else fused), (name, chain, p)
    return p
