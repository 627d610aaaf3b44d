"""CPU: the boundary-case generator (tests/boundary_cases.py) checked before the device sees its
cases. Three references that share no threshold form agree on every entry x every targeted disk,
the rational T equals the library's host build, and the cases have teeth: a `<` in place of the
`<=`, or a threshold one ulp too high, changes the expected area of every targeted candidate.

Reference: src/AreaCoverageCalculation.jl:63-78 (calculateArea: sqrt(dx^2 + dy^2) < r, first hit),
src/TDM_Constraints.jl:54-75 (cons3)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import boundary_cases as bc

_REF = {}


def _recs(x, y, w):
    return np.stack([x, y, w, w, np.zeros_like(x)], axis=1)


def _tables(name):
    """Per case, computed once: a[d, e] of every targeted disk d and entry e, T[d], the yardstick's
    decisions, and per targeted row the covered sets under the true and the two mutated predicates."""
    if name not in _REF:
        g = bc.make_case(name, "equal")
        ids = np.unique(g.disk_of)
        D = g.disks[ids]
        a = np.stack([bc.a_of(g.x, g.y, cx, cy) for cx, cy, _ in D])
        T = np.array([bc.threshold(r) for r in D[:, 2]])
        yard = np.sqrt(a) < D[:, 2][:, None]
        pos = {int(d): i for i, d in enumerate(ids)}
        _REF[name] = SimpleTables(g=g, ids=ids, D=D, a=a, T=T, yard=yard, pos=pos)
    return _REF[name]


class SimpleTables:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def row_cover(self, ri, mode):
        """Covered flags of targeted row ri under a <= T ("le"), a < T ("lt") or a <= next_up(T)
        ("up"), any disk."""
        sel = [self.pos[int(d)] for d in self.g.disk_of[ri]]
        a, T = self.a[sel], self.T[sel][:, None]
        if mode == "le":
            return (a <= T).any(0)
        if mode == "lt":
            return (a < T).any(0)
        return (a <= np.nextafter(T, np.inf)).any(0)


@pytest.mark.parametrize("name", bc.CASES)
def test_three_references_agree(orc, name):
    """(i) numpy sqrt(a) < r, (ii) the C oracle, (iii) the rational decision Fraction(a) < m^2 with
    m = (pred(r) + r) / 2 (no sqrt, no T) on every entry x every disk of every targeted candidate;
    the tie a == m^2 never occurs. (iii) runs in exact rationals wherever |a - r r| <= 2^-20 r r;
    outside that band fl(r r) and m^2 (both within 2^-51 r^2 of r^2) leave a margin 2^31 times their
    distance, and the comparison of a with fl(r r) is the rational one's."""
    t = _tables(name)
    g = t.g
    rec = _recs(g.x, g.y, np.full(g.x.size, 25.0))
    M = g.x.size
    for i, (cx, cy, r) in enumerate(t.D):
        # (ii) the C restatement's rmvCoveredPOI under this disk alone: what it removes is covered
        kept = orc.ref_remove_covered(np.array([cx, cy, r]), rec)
        c_cov = np.ones(M, dtype=bool)
        c_cov[kept] = False
        assert np.array_equal(c_cov, t.yard[i]), (name, i)
        # (iii)
        rr = r * r
        band = np.abs(t.a[i] - rr) <= rr * 2.0 ** -20
        rat = t.a[i] < rr
        m2 = ((Fraction(math.nextafter(r, 0.0)) + Fraction(r)) / 2) ** 2
        for e in np.flatnonzero(band):
            fa = Fraction(float(t.a[i, e]))
            assert fa != m2, (name, i, e)
            rat[e] = fa < m2
        assert np.array_equal(rat, t.yard[i]), (name, i, np.flatnonzero(rat != t.yard[i])[:5])
        # ... and the form the kernels decide, under the rational T
        assert np.array_equal(t.a[i] <= t.T[i], t.yard[i]), (name, i)
    # the oracles once more per candidate: flags and (both weight modes) areas
    for wt in bc.WEIGHTS:
        c = bc.make_case(name, wt)
        want = orc.PointerList(_recs(c.x, c.y, c.w)).area_batch(c.C[c.rows])
        for ri, k in enumerate(c.rows):
            cov = t.row_cover(ri, "le")
            if wt == "equal":
                assert np.array_equal(orc.np_covered(c.C[k], c.x, c.y), cov), (name, k)
            assert want[ri] == float(np.sum(c.w[cov])), (name, wt, k)   # (exact in any order)


@pytest.mark.parametrize("name", bc.CASES)
def test_rational_threshold_is_the_host_builds(pkg, name):
    g = bc.make_case(name, "equal")
    N = g.N
    for r in np.unique(g.C[:, 2 * N:]):
        assert bc.threshold(r) == pkg.cover_threshold(float(r)), r


@pytest.mark.parametrize("weights", bc.WEIGHTS)
@pytest.mark.parametrize("name", bc.CASES)
def test_cases_have_teeth(orc, name, weights):
    """Conditions, not measurements: the generator fails loudly where it cannot meet one."""
    t = _tables(name)
    c = bc.make_case(name, weights)
    N, M, K = c.N, c.x.size, c.K
    assert M <= 60000 and 64 <= K <= 243
    assert c.rows.size >= (16 if name in ("near", "crowded", "escaped") else 8)
    assert np.all(c.C[:, :] != np.round(c.C))          # no integer centre, no integer radius
    assert np.array_equal(c.C[0], c.prev)
    if weights == "equal":
        assert np.all(c.w == 25.0)
    else:
        assert set(np.unique(c.w)) == {1.0, 2.0, 4.0, 8.0}
    if name == "escaped":
        esc = ~c.packs.all(axis=1)
        assert K // 4 <= esc.sum() <= K // 2 and not esc[0]
        assert np.count_nonzero(esc[c.rows]) >= 4      # targets on the final, escaped disks
        assert (np.abs(c.C - c.C[0])[:, :2 * N] > 1023).any()
    else:
        assert c.packs.all()                           # real-valued incumbent, every key packs
    feas = orc.cons3_batch(c.prev, c.C, c.d_lim, bc.TAN50)
    assert K // 4 <= feas.sum() <= 3 * K // 4 and feas[0]

    # every targeted disk: decisive on and off entries
    if name != "crowded":
        assert c.exposed.all()
    n_on = n_off = 0
    changed = {"lt": 0, "up": 0}
    for ri, k in enumerate(c.rows):
        cx, cy, r = c.C[k, :N], c.C[k, N:2 * N], c.C[k, 2 * N:]
        for u in range(N):
            if name == "crowded" and bc.exposed_angles(u, cx, cy, r).size == 0:
                continue
            mine = np.flatnonzero(c.disk == c.disk_of[ri, u])
            oth = np.arange(N) != u
            dec = ~bc.covered_by(c.x[mine], c.y[mine], cx[oth], cy[oth], r[oth])
            a = t.a[t.pos[int(c.disk_of[ri, u])], mine]
            T = bc.threshold(r[u])
            on = dec & (c.cls[mine] == bc.ON)
            off = dec & (c.cls[mine] == bc.OFF)
            assert np.all(a[c.cls[mine] == bc.ON] == T)
            assert np.all(a[c.cls[mine] == bc.OFF] == math.nextafter(T, math.inf))
            assert on.sum() >= c.need and off.sum() >= c.need, (name, k, u, on.sum(), off.sum())
            n_on += int(on.sum())
            n_off += int(off.sum())
        # the mutations: `<` for `<=`, next_up(T) for T
        area = float(np.sum(c.w[t.row_cover(ri, "le")]))
        for mode in changed:
            changed[mode] += float(np.sum(c.w[t.row_cover(ri, mode)])) != area
    assert changed["lt"] == c.rows.size and changed["up"] == c.rows.size, (name, changed)
    assert c.need == (1 if name == "far" else 2)

    # the ladder: both signs in every octave, four rungs each
    lad_disks = np.unique(c.disk[c.cls == bc.LADDER])
    assert lad_disks.size == N + 2
    assert set(c.disk_of[0]) <= set(lad_disks)
    for d in lad_disks:
        e = np.flatnonzero((c.cls == bc.LADDER) & (c.disk == d))
        cxd, cyd, rd = c.disks[d]
        T = bc.threshold(rd)
        steps = (bc.a_of(c.x[e], c.y[e], cxd, cyd) - T) / np.spacing(T)
        for o in bc.LADDER_OCTAVES:
            for s in (-1.0, 1.0):
                n = np.count_nonzero((s * steps >= 2.0 ** o) & (s * steps < 2.0 ** (o + 1)))
                assert n >= bc.RUNGS, (name, d, o, s, n)
        assert np.abs(steps).min() >= 2 and np.abs(steps).max() * np.spacing(T) <= T * 2.0 ** -6

    # the corner rows: x0 with one UAV at the corner of the poll's displacement bound, on / off
    # entries on the rays where the annulus shortcut hands over to the tests
    u = c.corner_uav
    x0 = c.C[0]
    poll = c.C[1:1 + c.n_poll]
    Dx = np.abs(poll[:, u] - x0[u]).max()
    Dy = np.abs(poll[:, N + u] - x0[N + u]).max()
    Dl = (x0[2 * N + u] - poll[:, 2 * N + u]).max()
    Dr = (poll[:, 2 * N + u] - x0[2 * N + u]).max()
    assert min(Dx, Dy, Dl, Dr) >= 1.0
    for row, dr, dist in ((c.row_in, -Dl, x0[2 * N + u] - Dl - math.hypot(Dx, Dy)),
                          (c.row_out, Dr, x0[2 * N + u] + Dr + math.hypot(Dx, Dy))):
        diff = c.C[row] - x0
        assert np.count_nonzero(diff) == 3
        assert abs(diff[u]) == Dx and abs(diff[N + u]) == Dy and diff[2 * N + u] == dr
        ri = int(np.flatnonzero(c.rows == row)[0])
        mine = np.flatnonzero(c.ray & (c.disk == c.disk_of[ri, u]))
        assert {int(v) for v in c.cls[mine]} == {bc.ON, bc.OFF}
        d0 = np.hypot(c.x[mine] - x0[u], c.y[mine] - x0[N + u])
        assert np.all(np.abs(d0 - dist) < 0.02), (name, row, d0, dist)
        cx, cy, r = c.C[row, :N], c.C[row, N:2 * N], c.C[row, 2 * N:]
        oth = np.arange(N) != u
        assert not bc.covered_by(c.x[mine], c.y[mine], cx[oth], cy[oth], r[oth]).any()
    print(f"\n{name}/{weights}: M={M} K={K} rows={c.rows.size} on={int((c.cls == bc.ON).sum())} "
          f"off={int((c.cls == bc.OFF).sum())} ladder={int((c.cls == bc.LADDER).sum())} "
          f"decisive on/off={n_on}/{n_off} changed by '<': {changed['lt']}/{c.rows.size}, by "
          f"next_up(T): {changed['up']}/{c.rows.size}; generated in {c.seconds:.1f} s")


def test_generator_is_deterministic_and_cached():
    g = bc.make_case("big", "pow2")
    assert bc.make_case("big", "pow2") is g
    assert not g.x.flags.writeable and not g.C.flags.writeable
    saved = dict(bc._GEOM), dict(bc._CASE)
    bc._GEOM.clear()
    bc._CASE.clear()
    try:
        h = bc.make_case("big", "pow2")
        for k in ("x", "y", "w", "C", "cls", "disk", "rows"):
            assert np.array_equal(getattr(g, k), getattr(h, k)), k
    finally:
        bc._GEOM.update(saved[0])
        bc._CASE.update(saved[1])
