"""Polls on either side of every constant that routes a poll chain (tests/test_shape_edges.py checks
the table and the generator on the CPU, tests/test_gpu_shape_edges.py runs the device over the cases).

csrc/eval_plan.h eval_plan (the route maxcover.hip enqueue_eval takes) and the kernel headers choose
kernels, launch shapes and per-thread layouts from K (candidates) and N (UAVs):

  K < kPollMinK                  no poll chain (the per-candidate walk), unless the poll walk is forced
  K <= kFwMaxK + 1               the fused chain may run; thread 0 of fiw_kernel takes candidate kFwMaxK
  K <= kIndexMaxK + 1            the index takes 3 candidates per thread, <= kIndexMaxKWide + 1: 6,
                                 above: the identity map (and no packed keys: no fused chain)
  keys_ld(K)                     key rows padded to KEY_PAD
  fin2_kernel                    8 ceil(K / (8 kF2C)) blocks of kF2C candidates
  prep_kernel                    kPrepC candidates per workgroup
  prep_x_kernel                  kPrepCX per workgroup, the first K mod kPrepCX take one more; only when
                                 K mod kPrepCX <= K div kPrepCX (`xk`) and N <= kPrepU
  N <= kPrepU                    prep_x_kernel / gen_x; cons3 failures left out of the walk (`excl`);
                                 one block of UAVs per penalty chain
  N > kTiledMaxN                 the poll walk, whatever the algorithm option says
  8 ceil(N / 8) workgroups       fiw_kernel, the index, the poll walk: N mod 8 != 0 leaves idle ones
  generated sources              pair: K == 2 n, n % 4 == 0; gen_x: K == 6 N, N <= kPrepU

Every shape below is derived from the table. The inputs are lattice lists with integer disks (the
exact lattice count applies) whose rows are candidate 0 plus small integer offsets: on the mesh, so
the keys pack and the index's direct-mapped table holds them. Escaped keys, crowded polls and entries
at the ulp boundary have their own cases (list_cases.py, boundary_cases.py).

Deterministic (workloads.SplitMix64), numpy only, nothing read from outside the repository.
"""
import math
from types import SimpleNamespace

import numpy as np

import __graft_entry__ as ge

TAN50 = math.tan(100 / 180 * math.pi / 2)
CSRC = "maximumareacoverageoptimization.jl_amd/csrc/"

# name: (value, file, symbol). test_shape_edges.py reads the values back out of the sources.
CONSTANTS = {
    "kPollMinK": (64, CSRC + "maxcover.hip", "kPollMinK"),
    "kTiledMaxN": (2048, CSRC + "maxcover.hip", "kTiledMaxN"),
    "kFwThreads": (256, CSRC + "k_fiw.h", "kFwThreads"),
    "kFwMaxK": (3072, CSRC + "k_fiw.h", "kFwMaxK"),
    "kF2C": (16, CSRC + "k_fiw.h", "kF2C"),
    "kIndexMaxK": (3072, CSRC + "k_index.h", "kIndexMaxK"),
    "kIndexMaxKWide": (6144, CSRC + "k_index.h", "kIndexMaxKWide"),
    "kPrepU": (512, CSRC + "k_prep.h", "kPrepU"),
    "kPrepC": (8, CSRC + "k_prep.h", "kPrepC"),
    "kPrepCX": (6, CSRC + "k_prep.h", "kPrepCX"),
    "KEY_PAD": (32, CSRC + "k_prep.h", "keys_ld"),
    # AUTO's first matrix poll on a context starts on the five-launch chain when more than this
    # many of candidate 0's disks have a neighbour (maxcover.hip seed_route)
    "kBitsMinDisks": (16, CSRC + "k_common.h", "kBitsMinDisks"),
}
(kPollMinK, kTiledMaxN, kFwThreads, kFwMaxK, kF2C, kIndexMaxK, kIndexMaxKWide, kPrepU, kPrepC, kPrepCX,
 KEY_PAD, kBitsMinDisks) = (v[0] for v in CONSTANTS.values())

D_LIM = 10.0          # cons3's limit per UAV (src/FullSimulation.jl:740)
OFFSET = 3            # rows 1..K-1: candidate 0 + integer offsets in [-OFFSET, OFFSET]
FAIL_OFFSET = 8       # ... and on one row in FAIL_EVERY, +-8 in x and y of one UAV: cons3 fails
FAIL_EVERY = 8        # (sqrt(8^2 + 8^2) > 10 >= sqrt(3^2 + 3^2 + (3 / tan 50)^2))
ZERO_EVERY = 8        # r_max = candidate 0's radii + 0 or 1 per UAV, inside the offsets' range: the
#                       violations sum_i |d_i - a_i| are integers (exact), non-zero and different on
#                       most rows; one row in ZERO_EVERY has radii == r_max (violation 0)
WG_ALIGN = 8          # fiw_kernel, the index and the poll walk launch 8 ceil(N / 8) workgroups
#                       (eval_plan.h: nfw, nidx; maxcover.hip pgrid: one per XCD and disk group)
N_K = WG_ALIGN        # the N of K_EDGES and SMALL_K
ELL = 3               # GEN_N's mesh step 2^3 = 8


def _residue_case(start, r):
    """The first K >= start with K mod kPrepCX == r and no workgroup, block or key row full."""
    K = start
    while not (K % kPrepCX == r and K % kPrepC and K % kF2C and K % KEY_PAD):
        K += 1
    return K


# (K, what lies at it). N = N_K.
K_EDGES = (
    (kPollMinK - 1, "no poll chain under AUTO (forced chains included): the per-candidate walk"),
    (kPollMinK, "the first poll chain"),
    (kPollMinK + 1, "one candidate into the next key word, prep workgroup and fin2 block"),
    (kFwMaxK, "the fused chain's threads all full (kFwThreads x 12), no odd candidate"),
    (kFwMaxK + 1, "thread 0 of fiw_kernel takes candidate kFwMaxK; the last 3-per-thread index"),
    (kFwMaxK + 2, "no fused chain even when forced: disk_index_kernel, 6 per thread"),
    (kIndexMaxKWide, "the 6-per-thread index's threads all full"),
    (kIndexMaxKWide + 1, "its odd candidate"),
    (kIndexMaxKWide + 2, "the identity map, no keys"),
    (_residue_case(kPollMinK + 2, 2), "K mod kPrepCX == 2"),
    (_residue_case(2 * kPollMinK, 3), "K mod kPrepCX == 3"),
    (_residue_case(3 * kPollMinK, 4), "K mod kPrepCX == 4"),
)
K_WEIGHTED = (kFwMaxK + 1, kFwMaxK + 2, K_EDGES[-1][0])

# K = 1 .. 36 with the poll walk forced: below kPollMinK the only way into the chains. Crosses every
# flip of `xk` (5|6, 7|8, 11|12, 14|15, 17|18, 21|22, 23|24, 28|29, 29|30; no flip above 30) and the
# part-full blocks K < kPrepC, kF2C.
SMALL_K = tuple(range(1, kPrepCX * kPrepCX + 1))

K_FOR_N = _residue_case(kPollMinK, 4)     # 70: == 4 mod 6, == 6 mod 8, 16 and 32
# (N, what lies at it). K = K_FOR_N.
N_EDGES = (
    (1, "one disk: 7 of fiw's / the index's 8 workgroups idle, no second disk to share with"),
    (2, "the first shared entries"),
    (WG_ALIGN - 1, "one idle workgroup"),
    (WG_ALIGN, "no idle workgroup"),
    (WG_ALIGN + 1, "a second group of 8 workgroups, 7 idle; a third closure workgroup with one disk"),
    (kPrepU - 1, "prep_x_kernel with one idle thread; excl"),
    (kPrepU, "prep_x_kernel full; the last N with excl and a one-block penalty chain"),
    (kPrepU + 1, "prep_kernel, two UAV blocks; cons3 failures evaluated, then +inf"),
    (kTiledMaxN, "the last N the per-candidate walk holds: algo='tiled' is honoured"),
    (kTiledMaxN + 1, "the poll walk, whatever the algorithm option"),
)
N_WEIGHTED = (kPrepU, kPrepU + 1)

# basis-form polls (K = 6 N): (N, the generated-source prep layout it takes)
GEN_N = (
    (-(-kPollMinK // 6), "gen_x, the smallest N with 6 N >= kPollMinK"),
    (14, "gen_x; n = 42 is no multiple of 4"),
    (kPrepU - 1, "gen_x"),
    (kPrepU, "gen_x, the last"),
    (kPrepU + 1, "n = 1539: no pair, prep_kernel by candidates, two UAV blocks, K past the fused limit"),
    (kPrepU + 4, "n = 1548: pair"),
)


def xk(K, N=N_K):
    """The fused chain's matrix-source prep is prep_x_kernel (else prep_kernel)."""
    gx = K // kPrepCX
    return N <= kPrepU and gx >= 1 and K - gx * kPrepCX <= gx


def route(N, K, algo="auto", chain="auto", fresh=False):
    """What enqueue_eval launches for a matrix poll: (a poll chain runs, fiw_kernel runs). The
    second is None where AUTO's routing history decides (`fresh`: the context's first poll, which
    starts fused unless more than kBitsMinDisks of candidate 0's disks have neighbours).

    The launch roles cannot tell the 3- from the 6-per-thread index, prep_x_kernel from prep_kernel
    or excl from its absence: those are asserted on the plan itself (plan below)."""
    big = N > kTiledMaxN
    chain_runs = algo == "poll" or big or K >= kPollMinK
    keys = K <= kIndexMaxKWide + 1
    fused_ok = (chain_runs and keys and K <= kFwMaxK + 1 and chain != "five"
                and not (algo == "tiled" and not big))
    if not fused_ok:
        return chain_runs, False
    if chain == "fused" or (fresh and N <= kBitsMinDisks):
        return True, True
    return True, None


# mac_diag_route (csrc/maxcover.hip; host only): the plan's fields in the order it writes them
PLAN_FIELDS = ("poll_possible", "walk_forced", "iper", "want_keys", "pair", "gen_x", "mesh", "nchain", "G",
               "units", "fused_eligible", "excl", "counts", "prep_fused", "nprep", "xbase", "prep_five_runs",
               "prep_five", "nrec", "nfw", "nidx", "nfin2", "nfin")
PREP_KERNEL, PREP_X_MATRIX, PREP_X_GEN = 0, 1, 2       # eval_plan.h PrepKind
SRC_MATRIX, SRC_BASIS, SRC_GENERATED = 0, 1, 2         # eval_plan.h RouteIn::Kind


def plan(N, K, algo="auto", chain="auto", *, kind=SRC_MATRIX, np_=0, k0=0, mesh=False, mst=False,
         route_five=False, b=0, delta=0.0, want_area=False, want_obj=True, cons3=False, mask=False,
         tiled=True, cus=256, M=96 * 96, w_uniform=True):
    """The route the library plans for one evaluation (eval_plan.h eval_plan through mac_diag_route;
    no device): a namespace of PLAN_FIELDS. tiled: what use_tiled gives a device-resident poll."""
    import ctypes
    pkg = ge.load_package()
    L = pkg.load_library()
    L.mac_diag_route.argtypes = [ctypes.POINTER(ctypes.c_int64), ctypes.c_double,
                                 ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]
    L.mac_diag_route.restype = ctypes.c_int32
    args = (pkg._lib.ALGOS[algo], pkg._lib.CHAINS[chain], cus, M, w_uniform, kind, np_, k0, mesh, mst,
            route_five, b, want_area, want_obj, cons3, mask, tiled, N, K)
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    rc = L.mac_diag_route((ctypes.c_int64 * len(args))(*(int(a) for a in args)), float(delta), out, len(out))
    assert rc == 0, (rc, N, K)
    return SimpleNamespace(**dict(zip(PLAN_FIELDS, (int(v) for v in out))))


def grid_size(N):
    return 96 if N <= 64 else 256


_LIST = {}
_CASE = {}


def points(G, weighted, seed):
    """The G x G lattice list; weighted: weights from {1, 2, 4, 8} (every partial sum exact)."""
    key = (G, weighted, seed)
    if key not in _LIST:
        wl = ge.load_package().workloads
        x, y, w = wl.grid_points(G)
        if weighted:
            w = 2.0 ** wl.SplitMix64(seed + 7).integers(0, 3, x.size).astype(np.float64)
        for a in (x, y, w):
            a.setflags(write=False)
        _LIST[key] = (x, y, w)
    return _LIST[key]


def incumbent(N, G, rng, r_lo, r_hi):
    """Candidate 0: integer centres inside the list, integer radii in [r_lo, r_hi); disk 1 overlaps
    disk 0 (its centre half of disk 0's radius away)."""
    L = 5 * G
    m = 2 * r_hi
    cx = rng.integers(m, L - m, N).astype(np.float64)
    cy = rng.integers(m, L - m, N).astype(np.float64)
    R = rng.integers(r_lo, r_hi - 1, N).astype(np.float64)
    if N >= 2:
        cx[1] = cx[0] + R[0] // 2
        cy[1] = cy[0]
    return np.concatenate([cx, cy, R])


def make(N, K, *, weighted=False, seed=1, argmin_last=False):
    """One poll of K candidates of N disks, arrays read-only:
      x, y, w          the point list (lattice, G = 96 for N <= 64, else 256)
      C                K x 3N: row 0 integer disks, rows 1.. = row 0 + integer offsets in [-3, 3];
                       one row in 8 (k = 4 mod 8) moves one UAV by +-8 in x and y (cons3 fails): the
                       last UAV on the first such row, the one before on the next, ...; the last
                       row and row kFwMaxK never fail
      D                the offsets, C == C[0] + D
      r_max            candidate 0's radii + A, A in {0, 1} per UAV: row k's violation is
                       sum_i |D[k, 2N + i] - A[i]|, an integer. One row in 8 (k = 2 mod 8) has radii
                       == r_max (violation 0); the last row and row kFwMaxK have a violation > 0
      prev, d_lim, tan_half_fov    cons3's arguments (prev = candidate 0)
    argmin_last: the last row's radii are r_max and every other row's violation is > 0: the last
    row is the strict minimiser."""
    key = (N, K, weighted, seed, argmin_last)
    if key in _CASE:
        return _CASE[key]
    wl = ge.load_package().workloads
    G = grid_size(N)
    x, y, w = points(G, weighted, seed)
    rng = wl.SplitMix64(1000003 * seed + 4099 * N + K)
    x0 = incumbent(N, G, rng, *((10, 30) if N <= 64 else (4, 12)))
    A = rng.integers(0, 1, N)
    A[0] = 1                          # (candidate 0 has a violation of its own)
    D = rng.integers(-OFFSET, OFFSET, K * 3 * N).reshape(K, 3 * N)
    D[0] = 0
    sx = 2 * rng.integers(0, 1, K) - 1
    sy = 2 * rng.integers(0, 1, K) - 1
    for j, k in enumerate(range(FAIL_EVERY // 2, K, FAIL_EVERY)):
        if k not in (K - 1, kFwMaxK):
            who = (N - 1 - j) % N
            D[k, who] = sx[k] * FAIL_OFFSET
            D[k, N + who] = sy[k] * FAIL_OFFSET
    if argmin_last and K > 1:
        D[K - 1, :2 * N] = 0
        D[K - 1, 2 * N:] = A
        nonzero = np.arange(1, K - 1)
    else:
        for k in range(2, K - 1, ZERO_EVERY):
            D[k, 2 * N:] = A
        nonzero = np.array([k for k in (K - 1, kFwMaxK) if 1 <= k < K], dtype=np.int64)
    viol = np.abs(D[:, 2 * N:] - A[None, :]).sum(axis=1)
    fix = nonzero[viol[nonzero] == 0]
    D[fix, 2 * N] = A[0] - 1          # (a violation of 1)
    C = np.ascontiguousarray(x0[None, :] + D.astype(np.float64))
    c = SimpleNamespace(N=N, K=K, G=G, weighted=weighted, argmin_last=argmin_last, x=x, y=y, w=w,
                        C=C, D=D, A=A, r_max=x0[2 * N:] + A, prev=x0.copy(),
                        d_lim=np.full(N, D_LIM), tan_half_fov=TAN50)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASE[key] = c
    return c


def make_gen(N, *, seed=1):
    """A complete LTMADS poll in basis form at mesh step 2^ELL around an integer incumbent: L, rp,
    cp, delta (what poll_basis takes) and C, the 6N x 3N matrix the same products build. Radii in
    [10, 30) (N <= 64) or [10, 14): positive at every candidate."""
    key = ("gen", N, seed)
    if key in _CASE:
        return _CASE[key]
    wl = ge.load_package().workloads
    G = grid_size(N)
    x, y, w = points(G, False, seed)
    rng = wl.SplitMix64(7000003 * seed + 4099 * N)
    x0 = incumbent(N, G, rng, *((10, 30) if N <= 64 else (10, 14)))
    n = 3 * N
    Lm, rp, cp = wl.ltmads_basis_parts(n, ELL, rng)
    delta = 1.0
    B = Lm[rp][:, cp].astype(np.float64)
    C = np.ascontiguousarray(np.concatenate([x0[None, :] + delta * B.T, x0[None, :] - delta * B.T]))
    c = SimpleNamespace(N=N, K=2 * n, G=G, x=x, y=y, w=w, x0=x0, L=Lm, rp=rp, cp=cp, delta=delta, C=C,
                        r_max=np.full(N, 14.0 if N > 64 else 30.0), prev=x0.copy(),
                        d_lim=np.full(N, D_LIM), tan_half_fov=TAN50)
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASE[key] = c
    return c


def expected(orc, c, exact=True):
    """The oracle's values of a case: areas (the C oracle on the list; exact=False: 25 x the exact
    lattice count, equal weights only), objectives, cons3 feasibility, the objectives under cons3,
    and both argmins. Arrays read-only."""
    if exact:
        rec = np.stack([c.x, c.y, c.w, c.w, np.zeros_like(c.x)], axis=1)
        area = orc.PointerList(rec).area_batch(c.C)
    else:
        area = 25.0 * orc.lattice_count_batch(c.C, c.G).astype(np.float64)
    obj = -area + orc.violation_batch(c.C, c.r_max) * 1e5
    feas = orc.cons3_batch(c.prev, c.C, c.d_lim, c.tan_half_fov)
    bar = np.where(feas, obj, np.inf)
    for a in (area, obj, feas, bar):
        a.setflags(write=False)
    return SimpleNamespace(area=area, obj=obj, feas=feas, bar=bar, k=int(np.argmin(obj)),
                           k_bar=int(np.argmin(bar)))
