"""Point lists at the edges of the tile index (tests/test_list_cases.py checks the generator and the
sequences on the CPU; tests/test_gpu_list_edges.py and tests/test_gpu_list_sequences.py run every
device consumer of the index over them).

Every evaluation kernel reads the list through what build_index makes of it: the bounding box of the
finite entries, the tile pitch choose_grid picks for it, the tile keys, the tile-sorted copy and the
offsets. The cases here are lists whose index is degenerate or extreme: one tile, one row of tiles,
a pitch set by one far entry, a span that overflows a double or is subnormal, coordinates far from
the origin, non-finite entries, one tile holding most of the list, signed zeros, and a list longer
than one pass of the bounding-box kernel's grid.

Each case carries a poll of K = 2 * 3N + 1 = 67 candidates for N = 11 UAVs (the smallest poll that
takes the poll chains, kPollMinK = 64): the incumbent x0 and workloads.poll_candidates around it.
Weights are 25.0, or distinct powers of two where entries must be told apart: every partial sum is
exact in any order, so every comparison downstream is `==`.

The second half is list maintenance: a host model of the list (three numpy arrays; removal through
the oracle's rmvCoveredPOI) and scripted and seeded sequences of set / append / remove / regions
operations for the device to follow.

Deterministic (workloads.SplitMix64), numpy and the stdlib only; each case is built once per process.
"""
import math
from types import SimpleNamespace

import numpy as np

import __graft_entry__ as ge
from test_gpu_regions import ref_check, ref_override      # (the literal numpy restatements: no GPU)

TAN50 = math.tan(100 / 180 * math.pi / 2)
N = 11
K = 2 * 3 * N + 1
CASES = ("one_point", "two_points", "identical", "line_x", "line_y", "aspect", "outlier", "outlier_xy",
         "span_overflow_x", "span_overflow_xy", "subnormal_span", "offset", "nonfinite", "heavy_tile",
         "neg_zero", "wide_grid_stride", "outlier_1e30")
# Every entry of these lists gets the same decision from any disk (one position, or positions closer
# than any double distance resolves): a candidate covers all of them or none.
ALL_OR_NONE = ("one_point", "identical", "subnormal_span")
# These stay on the packed-key grid (integer moves of an integer incumbent): the fused chain runs.
FUSED = ("outlier", "heavy_tile", "nonfinite", "identical", "outlier_1e30")
BBOX_BLOCKS, BBOX_BLOCK = 1024, 256      # bbox_kernel: at most 1,024 workgroups of 256 entries a pass

_CASE = {}


def _wl():
    return ge.load_package().workloads


def lattice(n, pitch=5.0, ox=0.0, oy=0.0, m=None):
    """n x m entries (ox + (i + 1/2) pitch, oy + (j + 1/2) pitch), i outer."""
    m = n if m is None else m
    cx = ox + (np.arange(n, dtype=np.float64) + 0.5) * pitch
    cy = oy + (np.arange(m, dtype=np.float64) + 0.5) * pitch
    return np.repeat(cx, m), np.tile(cy, n)


def _disks(rng, x_lo, x_hi, y_lo, y_hi, r_lo, r_hi, n=N):
    """n disks, integer centres in the box and integer radii in [r_lo, r_hi], as [x; y; r]."""
    cx = np.floor(x_lo + rng.uniform(n) * (x_hi - x_lo))
    cy = np.floor(y_lo + rng.uniform(n) * (y_hi - y_lo))
    r = np.floor(r_lo + rng.uniform(n) * (r_hi - r_lo + 1))
    return np.concatenate([cx, cy, r])


def _poll(x0, rng, delta=1.0):
    C = np.concatenate([x0[None, :], _wl().poll_candidates(x0, rng, 2, delta, include_incumbent=False)])
    assert C.shape == (2 * x0.size + 1, x0.size)
    return np.ascontiguousarray(C)


def cons3_limit(C, x0):
    """A cons3 limit between two candidates' largest 3-D moves from x0, about half of them failing."""
    with np.errstate(invalid="ignore", over="ignore"):
        mv = np.zeros(C.shape[0])
        for u in range(N):
            dz = (C[:, 2 * N + u] - x0[2 * N + u]) / TAN50
            mv = np.maximum(mv, np.sqrt((C[:, u] - x0[u]) ** 2 + (C[:, N + u] - x0[N + u]) ** 2 + dz ** 2))
    s = np.sort(mv[np.isfinite(mv)])
    gaps = np.flatnonzero(s[1:] > s[:-1]) + 1
    j = gaps[np.argmin(np.abs(gaps - C.shape[0] // 2))]
    return float(0.5 * (s[j - 1] + s[j]))


def _gauss(rng, n):
    u1, u2 = rng.uniform(n), rng.uniform(n)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(2 * math.pi * u2)


def _build(name):
    wl = _wl()
    rng = wl.SplitMix64(9100 + CASES.index(name))
    delta, r_max, w, light, note = 1.0, 30.0 * TAN50, None, False, ""
    box = None            # a populated box for the region stats (x_lo, x_hi, y_lo, y_hi)
    if name == "one_point":
        x, y = np.array([50.0]), np.array([50.0])
        x0 = _disks(rng, 300, 500, 300, 500, 15, 30)
        x0[[0, N, 2 * N]] = (68.0, 50.0, 19.0)           # the entry sits near disk 0's circle
        box = (40.0, 60.0, 40.0, 60.0)
    elif name == "two_points":
        x, y = np.array([50.0, 80.0]), np.array([50.0, 50.0])
        x0 = _disks(rng, 300, 500, 300, 500, 15, 30)
        x0[[0, N, 2 * N]] = (45.0, 52.0, 20.0)           # entry 0 well inside disk 0
        x0[[1, N + 1, 2 * N + 1]] = (99.0, 50.0, 18.0)   # entry 1 just outside disk 1
        box = (40.0, 60.0, 40.0, 60.0)
    elif name == "identical":
        x, y = np.full(1500, 120.0), np.full(1500, 75.0)
        x0 = _disks(rng, 300, 500, 300, 500, 15, 30)
        x0[[0, N, 2 * N]] = (120.0, 93.0, 19.0)
        box = (100.0, 140.0, 60.0, 90.0)
    elif name in ("line_x", "line_y"):
        t = np.arange(700, dtype=np.float64) + 0.5
        c = np.full(700, 40.0)
        x, y = (t, c) if name == "line_x" else (c, t)
        along = np.floor(30 + 58 * np.arange(N) + 10 * rng.uniform(N))
        across = np.floor(36 + 9 * rng.uniform(N))
        r = np.floor(18 + 8 * rng.uniform(N))
        x0 = np.concatenate([along, across, r] if name == "line_x" else [across, along, r])
        box = (100.0, 300.0, 30.0, 50.0) if name == "line_x" else (30.0, 50.0, 100.0, 300.0)
    elif name == "aspect":
        x = np.round(_gauss(rng, 2000) * 1e6 * 1024) / 1024
        y = np.round(_gauss(rng, 2000) * 1e-3 * 2.0 ** 40) / 2.0 ** 40
        delta, r_max = 16384.0, 2.5e5
        cx = np.floor(-1.5e6 + 3e5 * np.arange(N) + 5e4 * rng.uniform(N))
        x0 = np.concatenate([cx, np.floor(2e4 * (rng.uniform(N) - 0.5)),
                             np.floor(1.1e5 + 4e4 * rng.uniform(N))])
        box = (-5e5, 5e5, -1.0, 1.0)
        note = "moves of 16384 m (delta): off the packed-key grid"
    elif name in ("outlier", "outlier_xy", "span_overflow_x", "span_overflow_xy", "outlier_1e30"):
        lx, ly = lattice(32)
        # outlier_1e30: S = 1e27, so the lattice lies 5e26 from its tile's centre: the fp32 offset is
        # finite and its square is not
        far = {"outlier": ([1e300], [80.0]), "outlier_xy": ([1e300], [-1e300]),
               "outlier_1e30": ([1e30], [80.0]),
               "span_overflow_x": ([-1.5e308, 1.5e308], [80.0, 80.0]),
               "span_overflow_xy": ([-1.5e308, 1.5e308], [-1.5e308, 1.5e308])}[name]
        at = 517                                         # (the far entries in the middle of the list)
        x = np.concatenate([lx[:at], far[0], lx[at:]])
        y = np.concatenate([ly[:at], far[1], ly[at:]])
        x0 = _disks(rng, 10, 150, 10, 150, 14, 26)
        box = (20.0, 90.0, 30.0, 120.0)
    elif name == "subnormal_span":
        x = np.where(rng.uniform(600) < 0.5, 0.0, 1e-310)
        x[:2] = (0.0, 1e-310)
        y = np.zeros(600)
        x0 = _disks(rng, 300, 500, 300, 500, 15, 30)
        x0[[0, N, 2 * N]] = (18.0, 0.0, 19.0)
        box = (-1.0, 1.0, -1.0, 1.0)
    elif name == "offset":
        p = 2.0 ** -5
        x, y = lattice(32, p, 2.0 ** 40, -2.0 ** 40)
        delta, r_max = p, 8 * p
        x0 = np.concatenate([2.0 ** 40 + np.floor(2 + 28 * rng.uniform(N)) * p,
                             -2.0 ** 40 + np.floor(2 + 28 * rng.uniform(N)) * p,
                             np.floor(5 + 4 * rng.uniform(N)) * p])
        box = (2.0 ** 40 + 4 * p, 2.0 ** 40 + 20 * p, -2.0 ** 40 + 6 * p, -2.0 ** 40 + 25 * p)
        note = "moves of 2^-5 m (delta): off the packed-key grid"
    elif name == "nonfinite":
        x, y = lattice(32)
        x, y = x.copy(), y.copy()
        w = np.full(x.size, 25.0)
        at = rng.permutation(x.size - 2)[:38] + 1
        at = np.concatenate([[0, x.size - 1], at])       # (the first and the last entry of the list too)
        nan, inf = math.nan, math.inf
        kinds = [(nan, None), (None, nan), (inf, None), (None, inf), (-inf, None), (None, -inf),
                 (nan, nan), (inf, -inf), (-inf, inf), (nan, inf)]
        for q, e in enumerate(at):
            vx, vy = kinds[q % len(kinds)]
            if vx is not None:
                x[e] = vx
            if vy is not None:
                y[e] = vy
            w[e] = 2.0 ** q
        x0 = _disks(rng, 10, 150, 10, 150, 14, 26)
        box = (20.0, 90.0, 30.0, 120.0)
    elif name == "heavy_tile":
        lx, ly = lattice(24)
        hx, hy = 62.5, 57.5                              # a lattice point, inside disks 3 and 7 of x0
        x = np.concatenate([lx, np.full(3000, hx)])
        y = np.concatenate([ly, np.full(3000, hy)])
        perm = rng.permutation(x.size)
        x, y = x[perm], y[perm]
        x0 = _disks(rng, 5, 115, 5, 115, 7, 10)
        x0[[3, N + 3, 2 * N + 3]] = (60.0, 60.0, 9.0)
        x0[[7, N + 7, 2 * N + 7]] = (66.0, 55.0, 10.0)
        box = (40.0, 90.0, 30.0, 80.0)
    elif name == "neg_zero":
        c = (np.arange(33, dtype=np.float64) - 16) * 5.0
        x, y = np.repeat(c, 33).copy(), np.tile(c, 33).copy()
        x[(x == 0) & (np.arange(x.size) % 2 == 0)] = -0.0
        y[(y == 0) & (np.arange(y.size) % 3 != 0)] = -0.0
        x0 = _disks(rng, -70, 70, -70, 70, 14, 26)
        x0[[0, N]] = (-0.0, 0.0)
        x0[[1, N + 1]] = (3.0, -0.0)
        box = (-30.0, 25.0, -0.0, 45.0)
    elif name == "wide_grid_stride":
        lx, ly = lattice(512)
        assert lx.size == BBOX_BLOCKS * BBOX_BLOCK
        # the bounding box's four extremes at positions >= 1024 * 256: seen by bbox_kernel's stride
        # loop alone
        x = np.concatenate([lx, [-50.0, 3000.0, 1282.5]])
        y = np.concatenate([ly, [-70.0, 2900.0, 1277.5]])
        x0 = _disks(rng, 300, 2300, 300, 2300, 250, 350)
        r_max = 300.0
        x0[[0, N, 2 * N]] = (-51.0, -69.0, 10.0)         # disks over the two extreme entries
        x0[[1, N + 1, 2 * N + 1]] = (3001.0, 2899.0, 10.0)
        light = True
    else:
        raise ValueError(name)
    if w is None:
        w = np.full(x.size, 25.0)
    C = _poll(x0, rng, delta)
    if name == "nonfinite":
        # infinite and huge finite radii among the candidates (off the packed-key grid, each alone in
        # its row)
        C[5, 2 * N + 2] = math.inf
        C[23, 2 * N + 6] = 1e300
        C[41, 2 * N] = 1e155
        C[58, 2 * N + 9] = math.inf
    r_max = np.full(N, float(r_max))
    d_lim = np.full(N, cons3_limit(C, x0))
    c = SimpleNamespace(name=name, N=N, K=K, x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), w=w, C=C,
                        r_max=r_max, prev=x0.copy(), d_lim=d_lim, box=box, light=light, note=note,
                        flag_rows=(0, K // 3, K - 1))
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def make_case(name):
    """The case `name` as a namespace, arrays read-only: x, y, w the list; C the K x 3N poll, row 0 the
    incumbent; r_max, prev, d_lim for the objective and cons3; box a populated region; flag_rows the
    candidates whose per-entry flags are compared; light: the largest list, few oracle calls."""
    if name not in _CASE:
        _CASE[name] = _build(name)
    return _CASE[name]


def recs(x, y, w):
    return np.stack([x, y, w, w, np.zeros_like(x)], axis=1)


def finite_bbox(x, y):
    """(xmn, xmx, ymn, ymx) of the finite coordinates, as bbox_kernel takes them (per axis)."""
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    inf = math.inf
    return (float(fx.min()) if fx.size else inf, float(fx.max()) if fx.size else -inf,
            float(fy.min()) if fy.size else inf, float(fy.max()) if fy.size else -inf)


def grid_cap(M):
    """The tile-count cap choose_grid documents: at most max(4M, 2^20) tiles, 2^28 in all."""
    return min(2.0 ** 28, max(4.0 * M, 2.0 ** 20))


# ------------------------------------------------------------------------------- list maintenance

class Model:
    """The list on the host: three arrays; with regions on, the importance override on incoming
    entries (src/CellFunctions.jl:42-45, :68-72) and the cumulative ingest counts."""

    def __init__(self, orc):
        self.orc = orc
        self.x = self.y = self.w = np.zeros(0)
        self.has_list = False            # (set or appended to at least once)
        self.boxes, self.w_high = None, math.nan
        self.cnt, self.tot = None, 0

    def _ingest(self, x, y, w, reset):
        x, y, w = (np.array(v, dtype=np.float64) for v in (x, y, w))
        if self.boxes is not None:
            m = ref_check(x, y, self.boxes)
            if reset:
                self.cnt, self.tot = np.zeros(m.shape[1], dtype=np.int64), 0
            self.cnt = self.cnt + m.sum(axis=0)
            self.tot += int(m.any(axis=1).sum())
            if self.w_high == self.w_high:
                w = ref_override(recs(x, y, w), self.boxes, self.w_high)[:, 3]
        return x, y, w

    def set(self, x, y, w):
        self.x, self.y, self.w = self._ingest(x, y, w, True)
        self.has_list = True

    def append(self, x, y, w):
        x, y, w = self._ingest(x, y, w, False)
        self.x, self.y, self.w = (np.concatenate(p) for p in ((self.x, x), (self.y, y), (self.w, w)))
        self.has_list = True

    def remove(self, circles):
        kept = self.orc.ref_remove_covered(circles, recs(self.x, self.y, self.w)) if self.x.size else \
            np.zeros(0, dtype=np.int64)
        self.x, self.y, self.w = self.x[kept], self.y[kept], self.w[kept]
        return kept

    def set_regions(self, boxes, w_high):
        self.boxes = tuple(np.asarray(v, dtype=np.float64) for v in boxes)
        self.w_high = float(w_high)
        self.cnt, self.tot = np.zeros(self.boxes[0].size, dtype=np.int64), 0

    def clear_regions(self):
        self.boxes, self.w_high, self.cnt, self.tot = None, math.nan, None, 0


SEQUENCES = ("stale_route", "mpc", "edges", "random1", "random2", "random3", "random4")
W_HIGH = 100.0            # 4 x 25: beside weights of 25 every partial sum stays exact
SEQ_BOXES = ([40.0, 200.0], [120.0, 260.0], [30.0, 150.0], [110.0, 240.0])
_SEQ = {}


def _state(rng, lo, hi, n=5, r_lo=14, r_hi=26):
    return _disks(rng, lo, hi, lo, hi, r_lo, r_hi, n)


def _cloud(rng, m, lo, hi):
    """m entries on the quarter-metre grid in [lo, hi)^2 (exact in fp32 too), weight 25."""
    q = 4 * (hi - lo)
    return (lo + np.floor(rng.uniform(m) * q) / 4, lo + np.floor(rng.uniform(m) * q) / 4, np.full(m, 25.0))


CROWDED_N = 24            # (more disks with neighbours than kBitsMinDisks = 16: the shared pass is hinted)


def _crowded_poll(rng, n=CROWDED_N):
    """n disks within a few metres of each other (K = 6 n + 1): every disk but the first has lower
    neighbours."""
    x0 = np.concatenate([np.floor(150 + 12 * rng.uniform(n)), np.floor(150 + 12 * rng.uniform(n)),
                         np.floor(18 + 8 * rng.uniform(n))])
    return _poll(x0, rng)


def _sparse_poll(rng, lo, hi):
    return _poll(_disks(rng, lo, hi, lo, hi, 14, 26), rng)


def _build_sequence(name):
    """A list of operations, each a dict: op ("set" | "append" | "remove" | "regions" | "clear_regions"
    | "polls": n polls of C through `paths` in turn), its arguments, and what follows it: probe (a
    5-disk state for flags, attribution and stats) and C (the K = 67 poll)."""
    wl = _wl()
    rng = wl.SplitMix64(7700 + SEQUENCES.index(name))
    ops = []
    lat = lattice(48)                                    # 2,304 entries over [0, 240)^2
    lat = (lat[0], lat[1], np.full(lat[0].size, 25.0))

    def add(op, **kw):
        kw.setdefault("probe", _state(rng, 20, 220))
        kw.setdefault("C", _sparse_poll(rng, 20, 220))
        ops.append(dict(op=op, **kw))

    if name == "stale_route":
        # twelve crowded polls on a dense list (the union pass gets its hint, the context its crowded
        # history), then a sparse list and a sparse poll on the same context, and back
        dense = lattice(64, 2.0, 90.0, 90.0)
        dense = (dense[0], dense[1], np.full(dense[0].size, 25.0))
        crowded = _crowded_poll(rng)
        sparse = _cloud(rng, 300, 0, 2000)
        sparse_C = _sparse_poll(rng, 100, 1900)
        add("set", how="set_points", pts=dense, C=crowded)
        add("polls", n=12, C=crowded, paths=(("poll", "five"),), expect_shared=True)
        add("set", how="set_points_device", pts=sparse, C=sparse_C,
            probe=_state(rng, 100, 1900, r_lo=60, r_hi=120))
        add("polls", n=3, C=sparse_C, probe=_state(rng, 100, 1900, r_lo=60, r_hi=120),
            paths=(("poll", "five"), ("auto", "auto"), ("poll", "fused")))
        add("set", how="set_points_records", pts=dense, C=crowded)
        add("polls", n=3, C=crowded, paths=(("auto", "auto"), ("poll", "five"), ("poll", "fused")))
        add("remove", circles=crowded[0], C=crowded)
        add("set", how="set_points_f32", pts=sparse, C=sparse_C,
            probe=_state(rng, 100, 1900, r_lo=60, r_hi=120))
        add("append", how="append_points", pts=dense, C=crowded)
        add("polls", n=2, C=sparse_C)
    elif name == "mpc":
        # append, then remove by the previous state: 12 steps on a 64 x 64 lattice revealed in bands
        gx, gy = lattice(64, 5.0)
        band = np.floor(gx / 5.0).astype(np.int64) // 6          # 11 bands of 6 columns (the last: 4)
        state = _state(rng, 20, 60)
        add("regions", boxes=SEQ_BOXES, w_high=W_HIGH)
        first = band == 0
        add("set", how="set_points", pts=(gx[first], gy[first], np.full(int(first.sum()), 25.0)))
        for t in range(1, 13):
            sel = band == min(t, 10)
            pts = (gx[sel], gy[sel], np.full(int(sel.sum()), 25.0))
            add("append", how="append_points_device" if t % 2 else "append_points", pts=pts, probe=state)
            add("remove", circles=state, probe=state)
            state = state.copy()
            state[:5] += np.floor(22 + 10 * rng.uniform(5))      # the swarm moves on with the front
            state[5:10] = np.floor(20 + 280 * rng.uniform(5))
            state[10:] = np.floor(14 + 12 * rng.uniform(5))
    elif name == "edges":
        empty = (np.zeros(0), np.zeros(0), np.zeros(0))
        add("append", how="append_points", pts=lat)              # onto a context that never had a list
        add("append", how="append_points", pts=empty)            # m = 0
        add("append", how="append_points_device", pts=(np.array([7.25]), np.array([300.5]), np.array([25.0])))
        add("remove", circles=np.zeros(0))                       # zero disks
        add("remove", circles=np.array([900.0, 900.0, 5.0]))     # a disk that covers nothing
        st = _state(rng, 30, 210)
        add("remove", circles=st, probe=st)
        add("remove", circles=st, probe=st)                      # the same circles again
        big = _cloud(rng, 2600, 0, 240)
        add("append", how="append_points_device", pts=big)       # more than doubles the list
        add("remove", circles=_state(rng, 30, 210))
        add("regions", boxes=SEQ_BOXES, w_high=W_HIGH)
        out = _cloud(rng, 40, 400, 700)
        add("append", how="append_points", pts=out, C=_sparse_poll(rng, 380, 700),
            probe=_state(rng, 400, 700, r_lo=40, r_hi=80))       # outside the bounding box
        add("remove", circles=_state(rng, 400, 700, r_lo=40, r_hi=80))
        add("remove", circles=np.array([0.0, 0.0, math.inf]))    # every finite entry goes
        add("append", how="append_points", pts=lat)              # onto the emptied list (regions on)
        add("remove", circles=_state(rng, 30, 210))
        add("clear_regions")
        add("append", how="append_points_device", pts=empty)
        st = _state(rng, 30, 210)
        add("remove", circles=st, probe=st)
        add("set", how="set_points_f32", pts=_cloud(rng, 1500, 0, 240))
        add("remove", circles=_state(rng, 30, 210))
    else:
        hows_set = ("set_points", "set_points_records", "set_points_device", "set_points_f32")
        hows_app = ("append_points", "append_points_device")
        model = Model(ge.load_oracle())                  # (the list's length steers the draws: M <= 5,000)

        def draw(op, **kw):
            add(op, **kw)
            apply_to_model(model, ops[-1])

        draw("set", how="set_points", pts=lat)
        regions = False
        for q in range(29):
            u = rng.uniform(1)[0]
            size = model.x.size
            if size > 3600:
                u *= 0.36
            if u < 0.36 and size > 0:
                st = _state(rng, 10, 230, r_lo=16, r_hi=34)
                draw("remove", circles=st, probe=st)
            elif u < 0.74:
                m = int(rng.integers(1, 900, 1)[0])
                draw("append", how=hows_app[q % 2], pts=_cloud(rng, m, 0, 240))
            elif u < 0.84:
                m = int(rng.integers(200, 2400, 1)[0])
                draw("set", how=hows_set[int(rng.integers(0, 3, 1)[0])], pts=_cloud(rng, m, 0, 240))
            elif u < 0.92:
                regions = not regions
                if regions:
                    draw("regions", boxes=SEQ_BOXES, w_high=W_HIGH)
                else:
                    draw("clear_regions")
            else:
                draw("polls", n=2)
    return ops


def make_sequence(name):
    if name not in _SEQ:
        _SEQ[name] = _build_sequence(name)
    return _SEQ[name]


def apply_to_model(model, op):
    """One operation on the host model; returns the kept indices for a removal."""
    kind = op["op"]
    if kind == "set":
        model.set(*op["pts"])
    elif kind == "append":
        model.append(*op["pts"])
    elif kind == "remove":
        return model.remove(op["circles"])
    elif kind == "regions":
        model.set_regions(op["boxes"], op["w_high"])
    elif kind == "clear_regions":
        model.clear_regions()
    elif kind != "polls":
        raise ValueError(kind)
    return None
