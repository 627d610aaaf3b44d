"""Crowded polls on either side of every chunk constant of the shared-entry passes (tests/
test_crowded_cases.py checks the table and the generator on the CPU, tests/test_gpu_crowded_edges.py
runs the device over the cases).

The kernels that decide the entries several disks' regions share loop over chunks:

  shared_or_kernel (k_or.h)          candidates kOrKC at a time, a disk's positions kOrTab at a time,
                                     kOrE entries per job
  shared_bits_kernel (k_bits.h)      candidates kBitsK per job; table groups of at most kBitsTab
                                     positions in at most kBitsGrp pieces (a disk's positions may be
                                     split over groups); the job's map values cached as uint16 when
                                     (1 + neighbours) x candidates <= kBitsUC; kBitsE entries staged at a
                                     time, kBitsWP x kWave per pass
  poll_shared_job (k_poll_shared.h)  kShC or kShCWide candidates per job
  coverage_poll_kernel (k_poll.h)    slices of kPollKPB positions over at most POLL_ROWS grid rows
  walk_setup_kernel (k_walk.h)       neighbour lists of kPollNbr; regions of 64 x 64 tiles

Every shape below is derived from the table. The polls are lattice lists with integer disks whose
rows are candidate 0 plus integer offsets (the keys pack, the exact lattice count applies), and a disk's
number of distinct positions is set exactly: row k of disk i takes combination k mod U_i of the disk's
own fixed enumeration of the offsets, so it has min(K, U_i) distinct (x, y, r) triples.

Deterministic (workloads.SplitMix64), numpy only, nothing read from outside the repository.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np

import __graft_entry__ as ge

TAN50 = math.tan(100 / 180 * math.pi / 2)
CSRC = "maximumareacoverageoptimization.jl_amd/csrc/"

# name: (value, file, symbol). test_crowded_cases.py reads the values back out of the sources.
CONSTANTS = {
    "kWave": (64, CSRC + "k_common.h", "kWave"),
    "kOrKC": (3584, CSRC + "k_or.h", "kOrKC"),
    "kOrTab": (4096, CSRC + "k_or.h", "kOrTab"),
    "kOrE": (64, CSRC + "k_or.h", "kOrE"),
    "kBitsK": (4096, CSRC + "k_bits.h", "kBitsK"),
    "kBitsTab": (2048, CSRC + "k_common.h", "kBitsTab"),
    "kBitsGrp": (4, CSRC + "k_bits.h", "kBitsGrp"),
    "kBitsUC": (16384, CSRC + "k_bits.h", "kBitsUC"),
    "kBitsUCMax": (65536, CSRC + "k_bits.h", "kBitsUCMax"),
    "kBitsE": (1024, CSRC + "k_bits.h", "kBitsE"),
    "kBitsWP": (2, CSRC + "k_bits.h", "kBitsWP"),
    "kShC": (64, CSRC + "k_poll_shared.h", "kShC"),
    "kShCWide": (256, CSRC + "k_poll_shared.h", "kShCWide"),
    "kPollKPB": (512, CSRC + "k_common.h", "kPollKPB"),
    # walk rows: min(POLL_ROWS, ceil(most positions of a disk / kPollKPB)) (maxcover.hip enqueue_five)
    "POLL_ROWS": (4, CSRC + "maxcover.hip", "gy"),
    "kPollNbr": (64, CSRC + "k_common.h", "kPollNbr"),
    "kBitsMinDisks": (16, CSRC + "k_common.h", "kBitsMinDisks"),
    "kIndexMaxKWide": (6144, CSRC + "k_index.h", "kIndexMaxKWide"),
    "kSharedWG": (256, CSRC + "k_common.h", "kSharedWG"),
}
(kWave, kOrKC, kOrTab, kOrE, kBitsK, kBitsTab, kBitsGrp, kBitsUC, kBitsUCMax, kBitsE, kBitsWP, kShC, kShCWide,
 kPollKPB, POLL_ROWS, kPollNbr, kBitsMinDisks, kIndexMaxKWide, kSharedWG) = (v[0] for v in CONSTANTS.values())
BITS_PASS = kBitsWP * kWave      # entries per pass of the bit-word kernel
REGION_TILES = 64                # a region wider or higher goes to the fp64 jobs (k_poll_shared.h neighbors_block)

# mac_diag_poll_report's counters (csrc/k_common.h kDc*), as _lib.POLL_COUNTERS names them
DC = ("bits", "poll_jobs", "other", "bits_jobs", "or_jobs0", "or_jobs1", "or_jobs2", "or_jobs3", "or_bad")

# ---------------------------------------------------------------------------- the base geometry
G_BASE = 64                      # 64 x 64 lattice at 5 m: 4,096 entries, tiles of about 10 m
N_BASE = 20
SQUARE = (112, 208)              # the centres' square (x and y); disks CORNERS sit on its corners
CORNERS = (15, 16, 17, 18)
R_RANGE = (15, 34)
R_LAST = 100
BOUND = (8, 8, 7)                # |dx|, |dy|, |dr| of the rows' integer offsets: 17 * 17 * 15 combinations
NCOMB = (2 * BOUND[0] + 1) * (2 * BOUND[1] + 1) * (2 * BOUND[2] + 1)
D_LIM = 12.0                     # cons3's limit: fails offsets such as (8, 8, 5), about one row in six
U_LARGE = tuple(NCOMB - i for i in range(N_BASE))   # 4335, 4334, ...: no two rows of a poll alike

# K axis (U_i = U_LARGE): either side of kOrKC, of kBitsK (= kOrTab), of the last K the index
# deduplicates, and two full candidate chunks of the union pass plus one
K_AXIS = (kOrKC, kOrKC + 1, kBitsK, kBitsK + 1, kIndexMaxKWide + 1, kIndexMaxKWide + 2, 2 * kOrKC + 1)
K_LAST = kBitsK + 1              # the K whose variants carry the strict last minimiser and cons3
# U axis at the last K the index deduplicates: positions per disk
K_U = kIndexMaxKWide + 1
U_AXIS = (1, 2, 3, 5,                                   # four consecutive disks: a group closes on kBitsGrp pieces
          kPollKPB - 1, kPollKPB, kPollKPB + 1,
          kBitsTab - 1, kBitsTab, kBitsTab + 1,
          kOrTab - 1, kOrTab, 3500,
          3001, 3038, 3075, 3112, 3149, 3186,
          kOrTab + 1)   # the last, large disk: its one position past kOrTab is the only disk on many entries
K_SMALL = 70                     # the hub and wide cases' K
K_U16 = kBitsUCMax + 64          # 65,600: the last kBitsK chunk is the 64 candidates past 2^16
N_U16 = 3

NAMES = (tuple(f"k{K}" for K in K_AXIS) + ("u_axis", "hub64", "hub65", "hubfirst65", "wide64", "wide65"))
VARIANTS = {"k%d" % K_LAST: ("last", "cons3"), "u_axis": ("last", "cons3"), "hub65": ("last", "cons3"),
            "wide65": ("last", "cons3")}

_CACHE = {}


def _lib():
    pkg = ge.load_package()
    L = pkg.load_library()
    L.mac_diag_grid.argtypes = [ctypes.c_double] * 4 + [ctypes.c_int64, ctypes.c_int32,
                                                        ctypes.POINTER(ctypes.c_double)]
    L.mac_diag_grid.restype = ctypes.c_int32
    L.mac_diag_tiles.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                 ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.mac_diag_tiles.restype = ctypes.c_int32
    return pkg, L


def grid(G):
    """The tile grid the library lays over the G x G lattice (host-only mac_diag_grid, default 4
    entries per tile): S, invS, nT (tiles per axis), g0 (the grid's origin on both axes)."""
    key = ("grid", G)
    if key not in _CACHE:
        pkg, L = _lib()
        x, y, _ = pkg.workloads.grid_points(G)
        out = (ctypes.c_double * 4)()
        assert L.mac_diag_grid(x.min(), x.max(), y.min(), y.max(), x.size, 4, out) == 0
        assert out[2] == out[3]
        _CACHE[key] = SimpleNamespace(S=out[0], invS=out[1], nT=int(out[2]), g0=float(x.min()), G=G)
    return _CACHE[key]


def points(G, weighted):
    """The lattice list; weighted: weights from {1, 2, 4, 8} (every partial sum exact), else all 25."""
    key = ("points", G, weighted)
    if key not in _CACHE:
        wl = ge.load_package().workloads
        x, y, w = wl.grid_points(G)
        if weighted:
            w = 2.0 ** wl.SplitMix64(4242 + G).integers(0, 3, x.size).astype(np.float64)
        for a in (x, y, w):
            a.setflags(write=False)
        _CACHE[key] = (x, y, w)
    return _CACHE[key]


def _combos(bound, rng, front=()):
    """A fixed enumeration of the integer offsets inside `bound`: (0, 0, 0) first, then `front`, then
    the rest in an order of the stream's."""
    bx, by, br = bound
    allc = [(a, b, c) for a in range(-bx, bx + 1) for b in range(-by, by + 1) for c in range(-br, br + 1)]
    head = [(0, 0, 0)] + [tuple(f) for f in front]
    taken = set(head)
    rest = [c for c in allc if c not in taken]
    perm = rng.permutation(len(rest))
    return np.array(head + [rest[p] for p in perm], dtype=np.int64)


def _offsets(K, U, bound, seed, front=()):
    """The rows' integer offsets D (K x 3N): disk i's row k is combination k mod U[i] of the disk's
    own enumeration."""
    wl = ge.load_package().workloads
    N = len(U)
    D = np.zeros((K, 3 * N), dtype=np.int64)
    k = np.arange(K)
    for i in range(N):
        comb = _combos(bound, wl.SplitMix64(seed * 1000003 + 7919 * i + 1), front)
        assert 1 <= U[i] <= len(comb), (i, U[i])
        d = comb[k % U[i]]
        D[:, i], D[:, N + i], D[:, 2 * N + i] = d[:, 0], d[:, 1], d[:, 2]
    return D


def _rows(x0, D):
    return np.ascontiguousarray(x0[None, :] + D.astype(np.float64))


def _base_x0(D, seed):
    """Candidate 0 of the base geometry: integer centres in SQUARE, integer radii in R_RANGE, the last
    disk R_LAST at the middle. A disk's radius is raised until its reach in each of the four directions
    (its radius + the largest offset its rows make that way) passes the square's middle by a metre, so
    every two regions overlap; a disk whose rows reach no further than 4 m is kept near the middle."""
    wl = ge.load_package().workloads
    rng = wl.SplitMix64(seed)
    N = N_BASE
    mid = (SQUARE[0] + SQUARE[1]) // 2
    cx = rng.integers(SQUARE[0], SQUARE[1], N).astype(np.float64)
    cy = rng.integers(SQUARE[0], SQUARE[1], N).astype(np.float64)
    R = rng.integers(R_RANGE[0], R_RANGE[1], N).astype(np.float64)
    cx[N - 1] = cy[N - 1] = mid
    for q, i in enumerate(CORNERS):   # (their regions carry the lower boxes' union to the square's full reach)
        cx[i], cy[i], R[i] = SQUARE[q & 1], SQUARE[q >> 1], R_RANGE[1]
    for i in range(N - 1):
        dx, dy, dr = D[:, i], D[:, N + i], D[:, 2 * N + i]
        slack = int(min((dx + dr).max(), (dr - dx).max(), (dy + dr).max(), (dr - dy).max()))
        if slack < 4:
            cx[i] = mid + (cx[i] - mid) // 8
            cy[i] = mid + (cy[i] - mid) // 8
        need = max(abs(cx[i] - mid), abs(cy[i] - mid)) + 1 - slack
        assert need <= R_RANGE[1], (i, need)
        R[i] = max(R[i], need)
    R[N - 1] = R_LAST
    return np.concatenate([cx, cy, R])


def _finish(name, G, x0, C, D, U, variant, d_lim, extra=None):
    N = len(U)
    wl = ge.load_package().workloads
    K = C.shape[0]
    if variant == "last":
        # r_max = the last row's radii: its violation is 0, every other row's an integer >= 1
        A = D[K - 1, 2 * N:].copy()
    else:
        A = wl.SplitMix64(31 + N + K).integers(0, 1, N)
        A[0] = 1
    c = SimpleNamespace(name=name, variant=variant, N=N, K=K, G=G, C=C, D=D, U=np.array(U, dtype=np.int64),
                        A=A, r_max=x0[2 * N:] + A, prev=x0.copy(), d_lim=np.asarray(d_lim, dtype=np.float64),
                        tan_half_fov=TAN50, cons3=variant == "cons3", **(extra or {}))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def targets(c):
    """ucount the index must report for the case's plain poll: the distinct triples per disk, or K for
    every disk under the identity map (K > kIndexMaxKWide + 1)."""
    if c.K > kIndexMaxKWide + 1:
        return np.full(c.N, c.K, dtype=np.int64)
    return np.minimum(c.K, c.U)


def _tile(g, v):
    """(tile of coordinate v, its distance to the nearer tile edge) on either axis."""
    u = (v - g.g0) / g.S
    t = math.floor(u)
    return t, min(u - t, t + 1 - u) * g.S


def _search(g, lo_tile, hi_tile, reach_extra, r_range):
    """Integer (centre, radius) whose reach [c - r - e, c + r + e] starts in tile lo_tile and ends in
    tile hi_tile, both ends at least 0.25 m from a tile edge."""
    for r in range(*r_range):
        for c in range(0, 5 * g.G):
            a, ma = _tile(g, c - r - reach_extra)
            b, mb = _tile(g, c + r + reach_extra)
            if (a, b) == (lo_tile, hi_tile) and ma >= 0.25 and mb >= 0.25:
                return float(c), float(r)
    raise AssertionError(("no integer disk spans tiles", lo_tile, hi_tile))


SMALL_BOUND = (1, 1, 1)
SMALL_FRONT = ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))   # every extreme of the reach, in every U >= 5
SMALL_R = 4


def _small_u(N):
    return [27 - (i % 4) for i in range(N)]


def _spots(g):
    """Integer centres of small disks (SMALL_R + offsets of 1: a reach of 6 m) whose boxes are the
    three tiles 3a .. 3a + 2 in x and 3b .. 3b + 2 in y: disjoint from one another."""
    axis = []
    for a in range(1, g.nT // 3 - 1):
        c, r = _search(g, 3 * a, 3 * a + 2, 2, (SMALL_R, SMALL_R + 1))
        axis.append(c)
    return [(cx, cy) for cy in axis for cx in axis]


def _hub(n_small, anchor):
    """A hub disk whose region overlaps n_small small, mutually disjoint disks of higher index; with
    `anchor`, a small disk of lower index inside the hub's region and disjoint from the rest, so that
    the hub itself has a lower neighbour."""
    g = grid(G_BASE)
    spots = _spots(g)
    assert len(spots) >= n_small + 1
    hub_c, hub_r = _search(g, 1, g.nT - 2, 2, (100, 160))
    cx, cy, R = [], [], []
    if anchor:
        cx.append(spots[-1][0]), cy.append(spots[-1][1]), R.append(float(SMALL_R))
    cx.append(hub_c), cy.append(hub_c), R.append(hub_r)
    for q in range(n_small):
        cx.append(spots[q][0]), cy.append(spots[q][1]), R.append(float(SMALL_R))
    return np.concatenate([cx, cy, R]), (1 if anchor else 0)


def _wide(tiles):
    """Eight disks on a larger lattice: disk 1's region is exactly `tiles` tiles wide and high and
    overlaps disk 0 (so it has a neighbour); disks 2 .. 7 are small disks inside it."""
    G = 144
    g = grid(G)
    assert g.nT >= tiles + 4
    wide_c, wide_r = _search(g, 2, 2 + tiles - 1, 2, (250, 400))
    spots = _spots(g)
    n = math.isqrt(len(spots))
    pick = [spots[b * n + a] for a, b in ((10, 10), (1, 1), (2, 1), (5, 15), (15, 5), (11, 10), (10, 11))]
    cx = [pick[0][0], wide_c] + [p[0] for p in pick[1:]]
    cy = [pick[0][1], wide_c] + [p[1] for p in pick[1:]]
    R = [float(SMALL_R), wide_r] + [float(SMALL_R)] * 6
    return G, np.concatenate([cx, cy, R])


def make(name, variant=""):
    """One poll, arrays read-only: N, K, G (the lattice), C (K x 3N), D (the integer offsets,
    C == C[0] + D), U (positions asked of each disk), r_max, prev / d_lim / tan_half_fov (cons3's
    arguments, used when c.cons3), and for the hub and wide cases `hub` / `wide` (that disk's index).
    variant "last": the last row is the strict minimiser; "cons3": the poll runs with cons3."""
    key = ("case", name, variant)
    if key in _CACHE:
        return _CACHE[key]
    seed = 77 + NAMES.index(name)
    if name.startswith("k") or name == "u_axis":
        K, U = (K_U, U_AXIS) if name == "u_axis" else (int(name[1:]), U_LARGE)
        D = _offsets(K, U, BOUND, seed)
        x0 = _base_x0(D, seed)
        C = _rows(x0, D)
        c = _finish(name, G_BASE, x0, C, D, U, variant, np.full(N_BASE, D_LIM))
    elif name.startswith("hub"):
        x0, hub = _hub(int(name[-2:]), anchor=not name.startswith("hubfirst"))
        N = x0.size // 3
        U = _small_u(N)
        D = _offsets(K_SMALL, U, SMALL_BOUND, seed, SMALL_FRONT)
        C = _rows(x0, D)
        d_lim = np.full(N, 10.0)
        d_lim[:4] = 1.5                      # fails (+-1, +-1, +-1) of the first four disks
        c = _finish(name, G_BASE, x0, C, D, U, variant, d_lim, dict(hub=hub))
    else:
        G, x0 = _wide(int(name[-2:]))
        N = x0.size // 3
        U = _small_u(N)
        D = _offsets(K_SMALL, U, SMALL_BOUND, seed, SMALL_FRONT)
        C = _rows(x0, D)
        d_lim = np.full(N, 10.0)
        d_lim[:4] = 1.5
        c = _finish(name, G, x0, C, D, U, variant, d_lim, dict(wide=1))
    _CACHE[key] = c
    return c


def make_u16():
    """K_U16 candidates of three mutually overlapping disks (the identity map: a position is the
    candidate's number, the last chunk's lie past 2^16)."""
    key = ("u16",)
    if key not in _CACHE:
        U = [NCOMB, NCOMB - 1, NCOMB - 2]
        x0 = np.array([150.0, 165.0, 160.0, 160.0, 150.0, 170.0, 30.0, 25.0, 34.0])
        D = _offsets(K_U16, U, BOUND, 5)
        C = _rows(x0, D)
        _CACHE[key] = _finish("u16", G_BASE, x0, C, D, U, "", np.full(N_U16, D_LIM))
    return _CACHE[key]


def regions(c):
    """Every disk's region as the device builds it: the union over the poll's rows of the disk's tile
    spans (predicate.h tile_span through the host-only mac_diag_tiles), int array [N][4] = {x lo, x hi,
    y lo, y hi}, lo > hi for a disk wholly off the grid."""
    key = ("regions", c.name)
    if key in _CACHE:
        return _CACHE[key]
    _, L = _lib()
    g = grid(c.G)
    out = (ctypes.c_int32 * 4)()
    span = {}

    def tiles(ctr, r):
        if (ctr, r) not in span:
            assert L.mac_diag_tiles(ctr, r, g.g0, g.invS, g.nT, out) == 0
            span[(ctr, r)] = (out[2], out[3]) if out[1] else None
        return span[(ctr, r)]
    N = c.N
    R = np.zeros((N, 4), dtype=np.int64)
    for i in range(N):
        box = [1 << 30, -1, 1 << 30, -1]
        for ax, col in ((0, i), (2, N + i)):
            for ctr, r in {(a, b) for a, b in zip(c.C[:, col].tolist(), c.C[:, 2 * N + i].tolist())}:
                s = tiles(ctr, r)
                if s:
                    box[ax] = min(box[ax], s[0])
                    box[ax + 1] = max(box[ax + 1], s[1])
        R[i] = box
    R.setflags(write=False)
    _CACHE[key] = R
    return R


def overlap(a, b):
    return a[0] <= b[1] and b[0] <= a[1] and a[2] <= b[3] and b[2] <= a[3]


def neighbours(c):
    """(lower, upper): per disk the indices of the lower- and higher-index disks whose regions overlap its."""
    R = regions(c)
    lo = [[j for j in range(i) if overlap(R[i], R[j])] for i in range(c.N)]
    up = [[j for j in range(i + 1, c.N) if overlap(R[i], R[j])] for i in range(c.N)]
    return lo, up


def counters(c, union_setup):
    """What walk_setup_kernel counts on the case (k_poll_shared.h neighbors_block): the disks with
    neighbours that qualify for the bit-word kernel and the union pass ("bits"), the others ("other":
    a lower list past kPollNbr, or a region past REGION_TILES tiles), and — counted only when the union
    pass's set-up runs — the disks with lower neighbours whose upper list is past kPollNbr ("or_bad")."""
    R = regions(c)
    lo, up = neighbours(c)
    out = dict(bits=0, other=0, or_bad=0)
    for i in range(c.N):
        if not lo[i]:
            continue
        bad = (len(lo[i]) > kPollNbr or R[i][1] - R[i][0] + 1 > REGION_TILES
               or R[i][3] - R[i][2] + 1 > REGION_TILES)
        out["other" if bad else "bits"] += 1
        if union_setup and len(up[i]) > kPollNbr:
            out["or_bad"] += 1
    return out


def shared_route(rep, bits_on, counts):
    """k_or.h shared_route on a report's counters: 0 the poll kernel's fp64 jobs, 1 the bit-word
    kernel, 2 the union pass."""
    nA, nB = rep["bits"], rep["other"]
    if not bits_on or nA + nB <= (0 if bits_on == 2 else kBitsMinDisks):
        return 0
    if not counts:
        return 1
    return 2 if nB == 0 and rep["or_bad"] == 0 else 0


def shared_entries(c, i):
    """The shared entries of disk i's job in the bit-word kernel (k_bits.h shared_runs): the list
    entries whose tile lies in region i and in a lower neighbour's region."""
    g = grid(c.G)
    R = regions(c)
    lo, _ = neighbours(c)
    x, y, _ = points(c.G, False)
    tx = np.floor((x - g.g0) * g.invS).astype(np.int64).clip(0, g.nT - 1)
    ty = np.floor((y - g.g0) * g.invS).astype(np.int64).clip(0, g.nT - 1)

    def inside(b):
        return (tx >= b[0]) & (tx <= b[1]) & (ty >= b[2]) & (ty <= b[3])
    m = np.zeros(x.size, dtype=bool)
    for j in lo[i]:
        m |= inside(R[j])
    return int(np.count_nonzero(m & inside(R[i])))


def bits_jobs(c):
    """The bit-word kernel's (disk, candidate chunk) jobs as its job loop cuts them: (disk, kb, kc,
    disks in the job, map values cached)."""
    lo, _ = neighbours(c)
    U = targets(c)
    out = []
    for i in range(c.N):
        if not lo[i]:
            continue
        nd = 1 + len(lo[i])
        for kb in range(0, c.K, kBitsK):
            kc = min(c.K, kb + kBitsK) - kb
            cached = nd * kc <= kBitsUC and all(U[d] <= kBitsUCMax for d in [i] + lo[i])
            out.append((i, kb, kc, nd, cached))
    return out


def expected(orc, c, weighted):
    """The C oracle's values of a case on the equal-weight or the weighted list: areas, objectives,
    cons3 feasibility, the objectives under cons3, both argmins. Arrays read-only."""
    x, y, w = points(c.G, weighted)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    area = orc.PointerList(rec).area_batch(c.C)
    obj = -area + orc.violation_batch(c.C, c.r_max) * 1e5
    feas = orc.cons3_batch(c.prev, c.C, c.d_lim, c.tan_half_fov)
    bar = np.where(feas, obj, np.inf)
    for a in (area, obj, feas, bar):
        a.setflags(write=False)
    return SimpleNamespace(area=area, obj=obj, feas=feas, bar=bar, k=int(np.argmin(obj)),
                           k_bar=int(np.argmin(bar)))
