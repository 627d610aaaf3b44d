"""Point lists whose entries sit exactly on, and one ulp beyond, the coverage thresholds of a poll's
own disks (tests/test_boundary_cases.py checks the generator on the CPU, tests/test_gpu_boundary.py
runs every device path over the cases).

The reference decides `sqrt(dx^2 + dy^2) < r` in fp64 (src/AreaCoverageCalculation.jl:70). With
a = fl(fl(dx dx) + fl(dy dy)) that is `a <= T(r)`, T(r) = RD(m^2), m = (pred(r) + r) / 2. T is
computed here from rationals (`threshold`), never by the library. For each targeted disk the
generator searches coordinates near the circle and keeps entries of four classes:

  on          a == T(r): covered, the last covered value
  off         a == next_up(T(r)): not covered, the first uncovered value
  ladder      a - T of both signs, from 2 ulps of T up to 2^-6 T, four rungs per octave, each rung
              at an angle of its own (row 0's disks and the two corner disks)
  background  a sparse lattice over the domain (and, in `far`, a few anchors at the origin)

The search is directed: per angle one coordinate is fixed (q = c_q + d sin t), the other solved
from the target (p = c_p +- sqrt(a* - dq^2)) and stepped by +-j ulps of p; both orientations are
tried, and half of the angles lie close to the disk's poles, where the solved offset is small and
one ulp of p moves `a` by less than one ulp of T (the only angles with a usable yield at coordinates
of 20,000 m).

The polls: C = [x0; x0 + B^T; x0 - B^T; the two corner rows], B an LTMADS basis on the unit mesh
(workloads.ltmads_basis_parts: the draws of workloads.poll_candidates), x0 real-valued with the low
mantissa bits of its values clear, so that x0 + d is exact for every mesh offset d and every key
packs (k_prep.h key_int), while no centre and no radius is an integer. `big` stacks three polls
(N = 4 gives 24 candidates each). The corner rows are x0 with one UAV moved to the corner of the
poll's displacement bound (largest |dx| and |dy| of that UAV over the poll, with the smallest,
respectively largest radius): no LTMADS direction reaches that corner itself (one variable per
direction carries the diagonal entry), and it is where the fused chain's annulus shortcut
(k_fiw.h) hands over to the tests. Their on / off entries lie on the ray from (x0, y0) that points
away from, respectively along, the displacement.

Deterministic (workloads.SplitMix64), numpy and the stdlib only, nothing read from outside the
repository; each case is built once per process.
"""
import math
import time
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import __graft_entry__ as ge

TAN50 = math.tan(100 / 180 * math.pi / 2)
CASES = ("near", "crowded", "far", "big", "escaped")
WEIGHTS = ("equal", "pow2")
BG, ON, OFF, LADDER = 0, 1, 2, 3
CLASS_NAMES = {BG: "background", ON: "on", OFF: "off", LADDER: "ladder"}
LADDER_OCTAVES = range(1, 46)    # |a - T| in [2^o, 2^(o+1)) ulps of T; 2^-6 T lies in octave 46
RUNGS = 4                        # per octave and sign
NEED = 2                         # decisive on and off entries per targeted disk (`far`: 1)

_T = {}
_GEOM = {}
_CASE = {}


def threshold(r: float) -> float:
    """T(r) = RD(m^2), m = (pred(r) + r) / 2, in exact rationals."""
    r = float(r)
    if r not in _T:
        if not (r > 0.0 and math.isfinite(r)):
            raise ValueError(r)
        m = (Fraction(math.nextafter(r, 0.0)) + Fraction(r)) / 2
        m2 = m * m
        t = m2.numerator / m2.denominator       # int / int: correctly rounded
        if Fraction(t) > m2:
            t = math.nextafter(t, 0.0)
        _T[r] = t
    return _T[r]


def quiet(v):
    """v with the low 8 mantissa bits clear: v + d stays exact for mesh offsets |d| < 2^8 ulp-wise
    (a sum that crosses into a higher binade drops low bits, which are zero here)."""
    a = np.ascontiguousarray(v, dtype=np.float64).copy()
    a.view(np.int64)[...] &= ~np.int64(0xFF)
    return a


def a_of(px, py, cx, cy):
    """a as the reference forms it: two products rounded, then their sum (numpy: no contraction)."""
    dx = px - cx
    dy = py - cy
    return dx * dx + dy * dy


def covered_by(px, py, cx, cy, r):
    """The yardstick sqrt(a) < r of the entries against any of the disks (cx, cy, r arrays)."""
    cov = np.zeros(np.shape(px), dtype=bool)
    for i in range(len(r)):
        cov |= np.sqrt(a_of(px, py, cx[i], cy[i])) < r[i]
    return cov


def exposed_angles(u, cx, cy, r, n=720, margin=0.01):
    """The sample angles (of n) at which disk u's circle lies outside every other disk by `margin`."""
    th = (np.arange(n) + 0.5) * (2 * math.pi / n)
    px = cx[u] + r[u] * np.cos(th)
    py = cy[u] + r[u] * np.sin(th)
    free = np.ones(n, dtype=bool)
    for i in range(len(r)):
        if i != u:
            free &= np.hypot(px - cx[i], py - cy[i]) > r[i] + margin
    return th[free]


def _trial(cx, cy, astar, th, J):
    """Trial coordinates around the circle a = astar about (cx, cy), one fixed and one solved
    coordinate per angle, the solved one stepped by -J..J ulps, in both orientations."""
    d = np.sqrt(astar)
    j = np.arange(-J, J + 1, dtype=np.float64)
    xs, ys, ks = [], [], []
    idx = np.arange(th.size)
    for swap in (False, True):
        cq, cp = (cx, cy) if swap else (cy, cx)
        sq, sp = (np.cos(th), np.sin(th)) if swap else (np.sin(th), np.cos(th))
        q = cq + d * sq
        dq = q - cq
        rem = astar - dq * dq
        ok = rem > 0.0
        p0 = cp + np.where(sp >= 0, 1.0, -1.0) * np.sqrt(np.where(ok, rem, 1.0))
        p = p0[:, None] + j[None, :] * np.spacing(np.abs(p0))[:, None]
        qq = np.broadcast_to(q[:, None], p.shape)
        kk = np.broadcast_to(idx[:, None], p.shape)
        p, qq, kk = p[ok].ravel(), qq[ok].ravel(), kk[ok].ravel()
        xs.append(qq if swap else p)
        ys.append(p if swap else qq)
        ks.append(kk)
    px, py = np.concatenate(xs), np.concatenate(ys)
    return px, py, a_of(px, py, cx, cy), np.concatenate(ks)


def _angles(rng, n, around=None, width=0.0):
    """n search angles: odd ones close to a pole (offset 10^-3.5 .. 10^-1 rad), even ones uniform,
    or, with `around`, drawn from those angles with a jitter of +-width."""
    u1, u2, u3 = rng.uniform(n), rng.uniform(n), rng.uniform(n)
    if around is not None and len(around):
        base = np.asarray(around)[np.minimum((u1 * len(around)).astype(np.int64), len(around) - 1)]
        uni = base + (2 * u2 - 1) * width
    else:
        uni = u1 * 2 * math.pi
    pole = np.floor(u1 * 4) * (math.pi / 2) + np.where(u3 < 0.5, -1.0, 1.0) * 10.0 ** (-1.0 - 2.5 * u2)
    return np.where(np.arange(n) % 2 == 1, pole, uni)


def _find_on_off(rng, u, cx, cy, r, need_on, need_off, around=None, width=0.0, only_around=False,
                 batches=24, n=1500):
    """Decisive on / off entries of disk u of the candidate (cx, cy, r): up to need_on / need_off of
    each, as two lists of (px, py). Decisive: no other disk of the candidate covers the entry."""
    T = threshold(r[u])
    Tn = math.nextafter(T, math.inf)
    oth = np.arange(len(r)) != u
    on, off = [], []
    for _ in range(batches):
        if len(on) >= need_on and len(off) >= need_off:
            break
        th = _angles(rng, n, around, width)
        if only_around:
            th = th[0::2]
        px, py, a, _ = _trial(cx[u], cy[u], T, th, 6)
        for val, lst, need in ((T, on, need_on), (Tn, off, need_off)):
            if len(lst) >= need:
                continue
            hit = np.flatnonzero(a == val)
            if hit.size:
                hit = hit[~covered_by(px[hit], py[hit], cx[oth], cy[oth], r[oth])]
            for h in hit:
                pt = (float(px[h]), float(py[h]))
                if pt not in lst and len(lst) < need:
                    lst.append(pt)
    return on, off


def _ladder(rng, cx, cy, r):
    """The ladder of one disk: per octave o of LADDER_OCTAVES, sign and rung, one entry with
    (a - T) / ulp(T) of that sign in [2^o, 2^(o+1)), each from angles of its own."""
    T = threshold(r)
    ulp = float(np.spacing(T))
    targets, lo, hi = [], [], []
    for o in LADDER_OCTAVES:
        for q in range(RUNGS):
            for s in (-1.0, 1.0):
                targets.append(T + s * ulp * 2.0 ** (o + (q + 0.5) / RUNGS))
                lo.append(s * 2.0 ** o)
                hi.append(s * 2.0 ** (o + 1))
    targets, lo, hi = np.array(targets), np.array(lo), np.array(hi)
    R = targets.size
    out = np.full((R, 2), np.nan)
    todo = np.arange(R)
    for _ in range(12):
        if not todo.size:
            break
        nang = 8
        th = _angles(rng, todo.size * nang)
        ast = np.repeat(targets[todo], nang)
        px, py, a, k = _trial(cx, cy, ast, th, 6)
        rung = todo[k // nang]
        e = (a - T) / ulp                    # exact: a - T is a multiple of ulp(T) / 2 at the least
        ok = (np.abs(e) >= np.abs(lo[rung])) & (np.abs(e) < np.abs(hi[rung])) & (np.sign(e) == np.sign(lo[rung]))
        hit = np.flatnonzero(ok)
        hit = hit[np.lexsort((np.abs(a[hit] - targets[rung[hit]]), rung[hit]))]
        first = hit[np.unique(rung[hit], return_index=True)[1]]   # per rung, the closest to its target
        out[rung[first], 0] = px[first]
        out[rung[first], 1] = py[first]
        todo = np.flatnonzero(np.isnan(out[:, 0]))
    if todo.size:
        raise RuntimeError(f"ladder: {todo.size} rungs of disk ({cx}, {cy}, {r}) found no entry")
    return out


_LAYOUT = {
    # name: (N, ell, polls, further targeted rows, background box and pitch, seed)
    "near":    dict(N=12, ell=1, polls=1, rows=15, box=(0.0, 1000.0, 0.0, 1000.0, 10.0), seed=7101),
    "crowded": dict(N=40, ell=2, polls=1, rows=15, box=(250.0, 550.0, 250.0, 550.0, 4.0), seed=7102),
    "far":     dict(N=12, ell=1, polls=1, rows=5, box=(19400.0, 20700.0, 17400.0, 18700.0, 12.5), seed=7103),
    "big":     dict(N=4, ell=3, polls=3, rows=5, box=(3400.0, 6600.0, 3400.0, 6600.0, 25.0), seed=7104),
    "escaped": dict(N=12, ell=1, polls=1, rows=15, box=(0.0, 2200.0, 0.0, 1000.0, 12.5), seed=7101),
}


def _pairs(rng, ox, oy, sx, sy, gap, along_x):
    """Six overlapping pairs on a 3 x 2 arrangement from (ox, oy) with steps (sx, sy): the radii of a
    pair within 1 m of each other, four of them k tan(50 deg) values that stay in their binade under
    the poll's moves."""
    first = [30 * TAN50, 20 * TAN50, 25 * TAN50, 14 * TAN50,
             float(quiet(17.3 + rng.uniform(1))[0]), float(quiet(21.0 + 9 * rng.uniform(1))[0])]
    cx, cy, r = [], [], []
    for p in range(6):
        bx = ox + (p % 3) * sx + 40 * rng.uniform(1)[0]
        by = oy + (p // 3) * sy + 40 * rng.uniform(1)[0]
        phi = 0.0 if along_x else rng.uniform(1)[0] * 2 * math.pi
        cx += [bx, bx + gap * math.cos(phi)]
        cy += [by, by + gap * math.sin(phi)]
        r += [first[p], min(first[p] + 0.2 + 0.6 * rng.uniform(1)[0], 35.9)]
    cx, cy, r = quiet(cx), quiet(cy), np.array(r)
    r[1::2] = quiet(r[1::2])
    return cx, cy, r


def _x0(name, rng):
    if name in ("near", "escaped"):
        cx, cy, r = _pairs(rng, 150.0, 230.0, 270.0, 420.0, 10.0, False)
    elif name == "far":
        cx, cy, r = _pairs(rng, 19650.0, 17700.0, 330.0, 520.0, 14.0, False)
    elif name == "crowded":
        N = 40
        cx = quiet(360.0 + 80.0 * rng.uniform(N))
        cy = quiet(360.0 + 80.0 * rng.uniform(N))
        r = quiet(15.0 + 20.9 * rng.uniform(N))
        r[[3, 17, 31]] = (30 * TAN50, 20 * TAN50, 15 * TAN50)   # (exact under moves of +-4)
    elif name == "big":
        # a chain across the diagonal: both ends of every disk's diagonal diameter (the corner rays)
        # lie outside the other three disks
        cx = quiet(np.array([4625.0, 4875.0, 5125.0, 5375.0]) + rng.uniform(4))
        cy = quiet(np.array([5375.0, 5125.0, 4875.0, 4625.0]) + rng.uniform(4))
        r = np.array([688 * TAN50, 820.0 * 1.003, 820.0 * 1.0007, 820.0 * 0.9991])
        r[1:] = quiet(r[1:])
    else:
        raise ValueError(name)
    return np.concatenate([cx, cy, r])


def packs(C):
    """Per value of C, whether its offset from row 0 packs into a key word (k_prep.h key_int: an
    integer within the field that reproduces the double from candidate 0's)."""
    N = C.shape[1] // 3
    lim = np.concatenate([np.full(2 * N, 1023.0), np.full(N, 511.0)])
    f = C - C[0]
    with np.errstate(invalid="ignore"):
        ok = (f >= -lim) & (f <= lim) & (np.trunc(f) == f) & (C[0] + np.trunc(f) == C)
    return ok


def _geometry(name):
    if name in _GEOM:
        return _GEOM[name]
    t0 = time.perf_counter()
    wl = ge.load_package().workloads
    L = _LAYOUT[name]
    N, ell = L["N"], L["ell"]
    n = 3 * N
    rng = wl.SplitMix64(L["seed"])
    x0 = _x0(name, rng)
    # the polls, in basis form (the first one's parts kept for mac_poll_basis_f64)
    blocks, basis = [], None
    for _ in range(L["polls"]):
        probe = wl.SplitMix64(0)
        probe.state = rng.state
        Lm, rp, cp = wl.ltmads_basis_parts(n, ell, rng)
        B = Lm[rp][:, cp].astype(np.float64)
        blk = np.concatenate([x0[None, :] + B.T, x0[None, :] - B.T])
        if not np.array_equal(blk, wl.poll_candidates(x0, probe, ell, include_incumbent=False)):
            raise RuntimeError("the basis form does not reproduce workloads.poll_candidates")
        blocks.append(blk)
        basis = basis or (Lm, rp, cp, 1.0)
    C = np.concatenate([x0[None, :]] + blocks)
    n_poll = C.shape[0] - 1
    moved = np.zeros(N, dtype=bool)
    if name == "escaped":
        # about a third of the candidates' values of UAVs 1, 4, 7, 10: off the mesh by 0.5 and by
        # 1e-9 (keys that no integer reproduces) and beyond the packed range (|dx| > 1023, |dr| > 511
        # would leave the radii's range: x only)
        for u, col, d in ((1, 1, 0.5), (4, N + 4, 1e-9), (7, 7, 1100.25), (10, 2 * N + 10, 0.5),
                          (10, N + 10, -0.5)):
            C[1 + (u % 3)::3, col] += d
            moved[u] = True
    # the corner rows, for every (UAV, signs): chosen below as the first whose ray entries exist
    srng = wl.SplitMix64(L["seed"] + 50)
    corner = None
    ray = {}
    for u in np.flatnonzero(~moved):
        Dx = np.abs(C[1:, u] - x0[u]).max()
        Dy = np.abs(C[1:, N + u] - x0[N + u]).max()
        Dl = (x0[2 * N + u] - C[1:, 2 * N + u]).max()
        Dr = (C[1:, 2 * N + u] - x0[2 * N + u]).max()
        for sx, sy in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
            rows = []
            for dr in (-Dl, Dr):
                c = x0.copy()
                c[u] += sx * Dx
                c[N + u] += sy * Dy
                c[2 * N + u] += dr
                rows.append(c)
            found = []
            for c, th0 in ((rows[0], math.atan2(-sy * Dy, -sx * Dx)), (rows[1], math.atan2(sy * Dy, sx * Dx))):
                on, off = _find_on_off(srng, u, c[:N], c[N:2 * N], c[2 * N:], 2, 2, around=[th0],
                                       width=0.03, only_around=True, batches=40, n=8000)
                found.append((on, off))
            if all(len(on) >= 1 and len(off) >= 1 for on, off in found):
                corner = (int(u), sx, sy, rows)
                ray = {"in": found[0], "out": found[1]}
                break
        if corner:
            break
    if corner is None:
        raise RuntimeError(f"{name}: no UAV has decisive on / off entries on both corner rays")
    C = np.ascontiguousarray(np.concatenate([C, np.stack(corner[3])]))
    K = C.shape[0]
    row_in, row_out = K - 2, K - 1
    pk = packs(C)
    if name != "escaped" and not pk.all():
        raise RuntimeError(f"{name}: {int((~pk).sum())} values do not pack")
    further = np.unique(np.round(np.linspace(1, n_poll, L["rows"])).astype(np.int64))
    rows = np.concatenate([[0], further, [row_in, row_out]])
    if name == "escaped":   # rows with escaped values among the targets
        esc_rows = np.flatnonzero(~pk[:n_poll + 1].all(axis=1))
        rows = np.unique(np.concatenate([rows, esc_rows[:: max(1, esc_rows.size // 6)][:6]]))
        rows = np.concatenate([rows[(rows != row_in) & (rows != row_out)], [row_in, row_out]])

    # ---- entries
    ent = []      # (px, py, class, disk id, ray)
    disks = {}    # (cx, cy, r) -> id

    def disk_id(c, u):
        return disks.setdefault((float(c[u]), float(c[N + u]), float(c[2 * N + u])), len(disks))

    need = 1 if name == "far" else NEED
    disk_of = np.zeros((rows.size, N), dtype=np.int64)
    exposed = np.zeros((rows.size, N), dtype=bool)
    by_disk = {}   # id -> [(px, py, class)]
    for kind, (on, off) in ray.items():
        c = C[row_in if kind == "in" else row_out]
        d = disk_id(c, corner[0])
        for cls, pts in ((ON, on), (OFF, off)):
            for p in pts:
                ent.append((p[0], p[1], cls, d, True))
                by_disk.setdefault(d, []).append((p[0], p[1], cls))
    for ri, k in enumerate(rows):
        c = C[k]
        cx, cy, r = c[:N], c[N:2 * N], c[2 * N:]
        for u in range(N):
            d = disk_id(c, u)
            disk_of[ri, u] = d
            arc = exposed_angles(u, cx, cy, r)
            exposed[ri, u] = arc.size > 0
            if not arc.size:
                if name != "crowded":
                    raise RuntimeError(f"{name}: disk {u} of row {k} has no arc of its own")
                continue
            # what the disk's entries from earlier rows already decide in this row
            have = by_disk.get(d, [])
            oth = np.arange(N) != u
            cnt = {ON: 0, OFF: 0}
            if have:
                hx = np.array([h[0] for h in have])
                hy = np.array([h[1] for h in have])
                dec = ~covered_by(hx, hy, cx[oth], cy[oth], r[oth])
                for h, ok in zip(have, dec):
                    cnt[h[2]] += bool(ok)
            on, off = _find_on_off(srng, u, cx, cy, r, max(0, need - cnt[ON]), max(0, need - cnt[OFF]),
                                   around=arc, width=math.pi / 720)
            if cnt[ON] + len(on) < need or cnt[OFF] + len(off) < need:
                raise RuntimeError(f"{name}: disk {u} of row {k}: {cnt[ON] + len(on)} on, "
                                   f"{cnt[OFF] + len(off)} off decisive entries, {need} needed")
            for cls, pts in ((ON, on), (OFF, off)):
                for p in pts:
                    ent.append((p[0], p[1], cls, d, False))
                    by_disk.setdefault(d, []).append((p[0], p[1], cls))
    ladder_disks = [disk_of[0, u] for u in range(N)] + [disk_id(C[row_in], corner[0]),
                                                        disk_id(C[row_out], corner[0])]
    inv = {v: k for k, v in disks.items()}
    for d in ladder_disks:
        cxd, cyd, rd = inv[d]
        for p in _ladder(srng, cxd, cyd, rd):
            ent.append((p[0], p[1], LADDER, d, False))
    x_lo, x_hi, y_lo, y_hi, pitch = L["box"]
    bx = x_lo + (np.arange(int((x_hi - x_lo) / pitch)) + 0.5) * pitch + 0.137
    by = y_lo + (np.arange(int((y_hi - y_lo) / pitch)) + 0.5) * pitch + 0.291
    gx, gy = np.repeat(bx, by.size), np.tile(by, bx.size)
    if name == "far":   # anchors at the origin: the index grid spans the whole range
        gx = np.concatenate([gx, [0.5, 1.25, 7.5, 3.0]])
        gy = np.concatenate([gy, [0.5, 3.75, 2.5, 11.0]])
    ex = np.concatenate([np.array([e[0] for e in ent]), gx])
    ey = np.concatenate([np.array([e[1] for e in ent]), gy])
    cls = np.concatenate([np.array([e[2] for e in ent], dtype=np.int8), np.zeros(gx.size, dtype=np.int8)])
    did = np.concatenate([np.array([e[3] for e in ent], dtype=np.int64), np.full(gx.size, -1, dtype=np.int64)])
    isray = np.concatenate([np.array([e[4] for e in ent], dtype=bool), np.zeros(gx.size, dtype=bool)])
    perm = wl.SplitMix64(L["seed"] + 99).permutation(ex.size)   # boundary entries all over the list
    disk_tab = np.array([inv[d] for d in range(len(disks))])
    # cons3: the limit between two candidates' largest 3-D moves, about half of them failing
    mv = np.zeros(K)
    for u in range(N):
        dz = (C[:, 2 * N + u] - x0[2 * N + u]) / TAN50
        mv = np.maximum(mv, np.sqrt((C[:, u] - x0[u]) ** 2 + (C[:, N + u] - x0[N + u]) ** 2 + dz ** 2))
    s = np.sort(mv)
    gaps = np.flatnonzero(s[1:] > s[:-1]) + 1            # s[j - 1] < s[j]
    j = gaps[np.argmin(np.abs(gaps - K // 2))]
    d_lim = float(0.5 * (s[j - 1] + s[j]))
    g = SimpleNamespace(
        name=name, N=N, ell=ell, x=ex[perm].copy(), y=ey[perm].copy(), cls=cls[perm].copy(),
        disk=did[perm].copy(), ray=isray[perm].copy(), C=C, K=K, n_poll=n_poll, basis=basis,
        rows=rows, row_in=row_in, row_out=row_out, corner_uav=corner[0], disk_of=disk_of,
        exposed=exposed, disks=disk_tab, packs=pk, need=need,
        r_max=np.full(N, float(np.max(x0[2 * N:])) if name == "big" else 30.0 * TAN50),
        prev=x0.copy(), d_lim=np.full(N, d_lim), seconds=time.perf_counter() - t0)
    for v in vars(g).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _GEOM[name] = g
    return g


def make_case(name, weights):
    """The case `name` under `weights` ("equal": all 25.0, "pow2": from {1, 2, 4, 8}, every partial
    sum exact) as a namespace, arrays read-only:
      x, y, w        the point list;            cls, disk, ray   per entry: class (BG / ON / OFF /
      C              K x 3N, row 0 = x0                          LADDER), targeted disk (row of
      r_max, prev, d_lim   the objective's and cons3's           `disks`, -1: none), on a corner ray
      rows           the targeted candidate rows (row_in, row_out: the corner rows, last)
      disk_of        rows x N: each targeted disk's row of `disks` ((cx, cy, r) per row)
      exposed        rows x N: the disk has an arc outside every other disk of its candidate
      n_poll, basis  C[1:1 + n_poll] is the poll of (L, rp, cp, delta) (the first 2n rows of it)
      packs          K x 3N: the value's key packs;      seconds   the geometry's generation time"""
    if (name, weights) not in _CASE:
        g = _geometry(name)
        M = g.x.size
        if weights == "equal":
            w = np.full(M, 25.0)
        elif weights == "pow2":
            wl = ge.load_package().workloads
            w = 2.0 ** wl.SplitMix64(_LAYOUT[name]["seed"] + 7).integers(0, 3, M).astype(np.float64)
        else:
            raise ValueError(weights)
        w.setflags(write=False)
        _CASE[(name, weights)] = SimpleNamespace(**vars(g), w=w, weights=weights)
    return _CASE[(name, weights)]
