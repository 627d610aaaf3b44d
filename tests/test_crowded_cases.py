"""CPU: the crowded-edge table and generator (tests/crowded_cases.py) checked before the device sees
the cases. The table equals the constants in the sources (a changed constant fails here, not by moving
an edge away from the tests); every disk has exactly the positions asked of it; the regions, neighbour
lists and job cuts the cases are meant to produce are restated from the kernels' arithmetic (the tile
spans through the host-only mac_diag_tiles) and hold; and every case has teeth: two references agree
on it, its areas differ from row to row, cons3 splits it, the strict last minimiser is one.

Reference: src/AreaCoverageCalculation.jl:63-78 (calculateArea), src/TDM_STATIC_opt.jl:82-100 (the
objective), src/TDM_Constraints.jl:54-75 (cons3)."""
import os
import re

import numpy as np
import pytest

import crowded_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXP = {}


def _exp(orc, name, variant="", weighted=False):
    key = (name, variant, weighted)
    if key not in _EXP:
        _EXP[key] = cc.expected(orc, cc.make(name, variant), weighted)
    return _EXP[key]


# ---------------------------------------------------------------------------- the table

def _source_constants():
    """Every `constexpr int NAME = EXPR;` of the table's files, evaluated: EXPR is made of integers,
    earlier names and * / + - << ( )."""
    text = {}
    for f in sorted({v[1] for v in cc.CONSTANTS.values()}):
        with open(os.path.join(ROOT, f)) as fh:
            text[f] = fh.read()
    raw = {}
    for t in text.values():
        for name, expr in re.findall(r"^\s*(?:static\s+)?constexpr\s+int\s+(\w+)\s*=\s*([^;,]+);", t, re.M):
            raw.setdefault(name, expr)

    def value(name, depth=0):
        expr = raw[name]
        assert depth < 8 and re.fullmatch(r"[\w\s*/+\-()<]+", expr), (name, expr)
        expr = re.sub(r"[A-Za-z_]\w*", lambda m: str(value(m.group(0), depth + 1)), expr)
        return int(eval(expr.replace("/", "//")))  # noqa: S307

    out = {}
    for key, (_, f, sym) in cc.CONSTANTS.items():
        if key == "POLL_ROWS":   # const int gy = std::max(1, std::min(4, (um_max + kPollKPB - 1) / kPollKPB));
            m = re.search(r"const int " + sym + r" = std::max\(1, std::min\((\d+), \(um_max \+ kPollKPB - 1\) / kPollKPB\)\);",
                          text[f])
            assert m, "the walk rows changed their form: update crowded_cases.CONSTANTS"
            out[key] = int(m.group(1))
        else:
            assert re.search(r"constexpr\s+int\s+" + sym + r"\b", text[f]), (sym, "not defined in", f)
            out[key] = value(sym)
    # the report's counter names, in the sources' order
    dc = dict(re.findall(r"\b(kDc[A-Z]\w*) = (\d+|kDcOrJobs \+ kOrBuckets)", text[cc.CSRC + "k_common.h"]))
    return out, dc


def test_table_equals_the_sources(pkg):
    got, dc = _source_constants()
    for key, (val, f, sym) in cc.CONSTANTS.items():
        assert got[key] == val, (f"tests/crowded_cases.py CONSTANTS[{key!r}] = {val}, but {f} has {sym} = "
                                 f"{got[key]}: update the table (its shapes follow) with the source")
    assert (dc["kDcBits"], dc["kDcPollJobs"], dc["kDcOther"], dc["kDcBitsJobs"], dc["kDcOrJobs"]) == \
        ("0", "1", "2", "3", "4") and dc["kDcOrBad"] == "kDcOrJobs + kOrBuckets"
    assert cc.DC == pkg._lib.POLL_COUNTERS and cc.DC.index("or_bad") == 4 + 4
    assert (cc.DC.index("bits"), cc.DC.index("other")) == (0, 2)


def test_report_rejects_bad_arguments_without_gpu(pkg):
    L = pkg.load_library()
    words = (pkg._lib._i32 * 10)()
    assert L.mac_diag_poll_report(None, words, 10, None, 0) == pkg._lib.MAC_E_INVAL
    assert "null" in L.mac_last_error().decode()


def test_shapes_sit_on_the_edges():
    assert cc.K_AXIS == (3584, 3585, 4096, 4097, 6145, 6146, 7169)
    assert cc.kOrTab == cc.kBitsK            # (one K edge serves both)
    assert cc.K_U == 6145 and cc.K_SMALL == 70 and cc.K_U16 == 65600
    assert cc.U_AXIS[:12] == (1, 2, 3, 5, 511, 512, 513, 2047, 2048, 2049, 4095, 4096) and cc.U_AXIS[-1] == 4097
    assert all(u >= 3000 for u in cc.U_AXIS[12:]) and len(cc.U_AXIS) == cc.N_BASE == 20
    assert cc.NCOMB == 4335 and min(cc.U_LARGE) > cc.kOrTab
    # K = 7169 is a third candidate chunk of the union pass and a second of the bit-word kernel
    assert -(-7169 // cc.kOrKC) == 3 and -(-7169 // cc.kBitsK) == 2
    assert cc.BITS_PASS == 128


# ---------------------------------------------------------------------------- the generator

@pytest.mark.parametrize("name", cc.NAMES)
def test_positions_per_disk_are_the_targets(name):
    """Distinct (x, y, r) triples per disk == min(K, U_i); integer disks; rows = row 0 + D, inside the
    packed keys' range; no two rows alike (the strict last minimiser depends on it)."""
    c = cc.make(name)
    N = c.N
    assert np.array_equal(c.C, np.rint(c.C)) and np.array_equal(c.C, c.C[0] + c.D)
    assert np.abs(c.D[:, :2 * N]).max() <= 1023 and np.abs(c.D[:, 2 * N:]).max() <= 511
    assert c.C[:, 2 * N:].min() >= 1
    for i in range(N):
        tri = np.stack([c.C[:, i], c.C[:, N + i], c.C[:, 2 * N + i]], axis=1)
        assert np.unique(tri, axis=0).shape[0] == min(c.K, c.U[i]), (name, i)
    assert np.unique(c.C, axis=0).shape[0] == c.K
    want = np.full(N, c.K) if c.K > cc.kIndexMaxKWide + 1 else np.minimum(c.K, c.U)
    assert np.array_equal(cc.targets(c), want)


def test_u_axis_lies_on_either_side_of_every_position_chunk():
    t = cc.targets(cc.make("u_axis")).tolist()
    for edge in (cc.kPollKPB, cc.kBitsTab, cc.kOrTab):
        assert {edge - 1, edge, edge + 1} <= set(t), edge
    assert t[:4] == [1, 2, 3, 5] and sum(t[:4]) < cc.kBitsTab    # a group closed by kBitsGrp pieces
    assert max(t) > cc.POLL_ROWS * cc.kPollKPB                     # more slices than the grid has rows
    # the K axis: U = K up to 4335 - i, then the identity map
    for K in cc.K_AXIS:
        u = cc.targets(cc.make(f"k{K}"))
        assert np.array_equal(u, np.full(20, K) if K <= 4097 or K > 6145 else np.array(cc.U_LARGE)), K


@pytest.mark.parametrize("name", [n for n in cc.NAMES if n[0] in "ku"])
def test_base_geometry_is_crowded(name):
    """Disk i has i lower neighbours (every two regions overlap): all lists fit, more than
    kBitsMinDisks disks have neighbours, no region is past 64 tiles: both passes take every disk."""
    c = cc.make(name)
    lo, up = cc.neighbours(c)
    assert [len(v) for v in lo] == list(range(c.N))
    assert cc.counters(c, True) == dict(bits=c.N - 1, other=0, or_bad=0)
    assert c.N - 1 > cc.kBitsMinDisks and c.N - 1 <= cc.kPollNbr
    x0 = c.C[0]
    assert x0[:2 * c.N].min() >= cc.SQUARE[0] and x0[:2 * c.N].max() <= cc.SQUARE[1]
    assert np.all((x0[2 * c.N:-1] >= cc.R_RANGE[0]) & (x0[2 * c.N:-1] <= cc.R_RANGE[1])) and x0[-1] == cc.R_LAST
    # the last disk's job in the bit-word kernel re-stages its entries: more than kBitsE + one pass
    assert cc.shared_entries(c, c.N - 1) > cc.kBitsE + cc.BITS_PASS


def test_bits_jobs_take_both_map_paths():
    """At K = kBitsK and kBitsK + 1 the (disk, chunk) jobs of the bit-word kernel fall on both sides of
    nd * kc <= kBitsUC (the job loop's arithmetic restated): the cached and the uncached map path."""
    for K in (cc.kBitsK, cc.kBitsK + 1):
        jobs = cc.bits_jobs(cc.make(f"k{K}"))
        assert {j[4] for j in jobs} == {True, False}, K
        assert len(jobs) == 19 * -(-K // cc.kBitsK)
    jobs = cc.bits_jobs(cc.make(f"k{cc.kBitsK + 1}"))
    assert any(kc == 1 and cached and nd == 20 for _, kb, kc, nd, cached in jobs)       # a one-candidate chunk
    assert any(kc == cc.kBitsK and nd * kc == cc.kBitsUC for _, kb, kc, nd, cached in jobs)   # the last cached job
    # positions past 2^16: every job of the uint16 case would fit the cache by size; none may take it
    c = cc.make_u16()
    jobs = cc.bits_jobs(c)
    assert jobs and all(nd * kc <= cc.kBitsUC and not cached for _, kb, kc, nd, cached in jobs)
    assert c.K - 1 >= cc.kBitsUCMax and [len(v) for v in cc.neighbours(c)[0]] == [0, 1, 2]


@pytest.mark.parametrize("name", ["hub64", "hub65", "hubfirst65"])
def test_hub_construction(name):
    """The hub's region overlaps every small disk's; the small disks' regions are mutually disjoint and
    disjoint from the anchor's: each has exactly one lower neighbour, the hub 64 or 65 upper ones. The
    union pass stands down (or_bad) only when a disk WITH a lower neighbour overflows its upper list:
    the hub behind an anchor disk does, a hub that is disk 0 does not (it owns no shared entry)."""
    c = cc.make(name)
    n = int(name[-2:])
    lo, up = cc.neighbours(c)
    R = cc.regions(c)
    h = c.hub
    assert len(up[h]) == n and lo[h] == ([0] if h else [])
    for i in range(h + 1, c.N):
        assert lo[i] == [h] and up[i] == [], (name, i)
    if h:
        assert lo[0] == [] and up[0] == [h]
    assert R[h][1] - R[h][0] + 1 <= cc.REGION_TILES and R[h][3] - R[h][2] + 1 <= cc.REGION_TILES
    want = dict(bits=c.N - 1, other=0, or_bad=1 if (h and n > cc.kPollNbr) else 0)
    assert cc.counters(c, True) == want and c.N - 1 > cc.kBitsMinDisks
    assert cc.shared_route(want, 2, 1) == (0 if want["or_bad"] else 2)


@pytest.mark.parametrize("name", ["wide64", "wide65"])
def test_wide_construction(name):
    c = cc.make(name)
    n = int(name[-2:])
    R = cc.regions(c)
    lo, _ = cc.neighbours(c)
    g = cc.grid(c.G)
    assert R[c.wide][1] - R[c.wide][0] + 1 == n and R[c.wide][3] - R[c.wide][2] + 1 == n
    assert R[c.wide][0] > 0 and R[c.wide][1] < g.nT - 1       # (inside the grid: not clamped to it)
    assert lo[c.wide] == [0] and all(lo[i] == [c.wide] for i in range(2, c.N))
    wide = n > cc.REGION_TILES
    assert cc.counters(c, True) == dict(bits=c.N - 1 - wide, other=int(wide), or_bad=0)
    assert cc.shared_route(cc.counters(c, True), 2, 1) == (0 if wide else 2)
    assert cc.shared_route(cc.counters(c, False), 2, 0) == 1


# ---------------------------------------------------------------------------- the cases' teeth

@pytest.mark.parametrize("name", cc.NAMES)
def test_two_references_agree_and_the_rows_differ(orc, name):
    c = cc.make(name)
    e = _exp(orc, name)
    cnt = orc.lattice_count_batch(c.C, c.G)
    assert np.array_equal(e.area, 25.0 * cnt.astype(np.float64)), name
    assert np.unique(e.area).size >= (8 if c.K == cc.K_SMALL else 50), name
    # the rows past every chunk edge are no copies of earlier ones
    assert e.area[-1] != e.area[0]
    ew = _exp(orc, name, weighted=True)
    x, y, w = cc.points(c.G, True)
    assert np.array_equal(w, np.rint(w)) and set(np.unique(w)) == {1.0, 2.0, 4.0, 8.0} and w.sum() < 2.0 ** 53
    assert np.array_equal(ew.area, np.rint(ew.area)) and not np.array_equal(ew.area, e.area)


@pytest.mark.parametrize("name", sorted(cc.VARIANTS))
def test_variants_have_teeth(orc, name):
    """"last": the last row is the strict minimiser (a dropped last candidate shows in the argmin);
    "cons3": the limit fails some rows and keeps others, and moves the argmin's objective."""
    c = cc.make(name, "last")
    for weighted in (False, True):
        e = _exp(orc, name, "last", weighted)
        assert e.k == c.K - 1 and np.count_nonzero(e.obj == e.obj[e.k]) == 1, (name, weighted)
    c = cc.make(name, "cons3")
    e = _exp(orc, name, "cons3")
    frac = e.feas.mean()
    assert c.cons3 and 0.05 < frac < 0.95 and e.feas[0], (name, frac)
    assert np.isinf(e.bar).sum() == np.count_nonzero(~e.feas) > 0


def test_u_axis_last_position_past_the_table_chunk_matters(orc):
    """The large last disk has kOrTab + 1 positions; its last one serves candidate kOrTab alone, and
    that candidate loses area when the disk is taken away: a table chunk dropped after the first
    (positions >= kOrTab) shows in the sum."""
    c = cc.make("u_axis")
    k, i = cc.kOrTab, c.N - 1
    assert c.U[i] == cc.kOrTab + 1 and np.flatnonzero(np.arange(c.K) % c.U[i] == k).tolist() == [k]
    row = c.C[k].copy()
    row[i] += 1000.0           # the disk moved off the list
    x, y, w = cc.points(c.G, False)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    without = orc.PointerList(rec).area_batch(row[None, :])[0]
    assert without < _exp(orc, "u_axis").area[k] - 25.0 * cc.kOrE


def test_uint16_case(orc):
    """The candidates past 2^16 are no copies of the positions a 16-bit cache would alias them to."""
    c = cc.make_u16()
    e = cc.expected(orc, c, True)
    tail = np.arange(cc.kBitsUCMax, c.K)
    assert tail.size == 64 and np.count_nonzero(e.area[tail] != e.area[tail - cc.kBitsUCMax]) > 32
