"""CPU: the shape-edge table and generator (tests/shape_edges.py) checked before the device sees the
cases. The table equals the constants in the sources (a changed constant fails here, not by moving an
edge away from the tests), every shape sits where the table says, and every case has teeth: two
references agree on it, its areas differ, cons3 splits it, disks share entries, and the mutations a
wrong edge would cause (the last candidate dropped from the argmin, candidate kFwMaxK read from a
stale slot) change the expected values.

Reference: src/AreaCoverageCalculation.jl:63-78 (calculateArea), src/TDM_STATIC_opt.jl:82-100 (the
objective), src/TDM_Constraints.jl:54-75 (cons3)."""
import os
import re

import numpy as np
import pytest

import shape_edges as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EXP = {}


# ---------------------------------------------------------------------------- the table

def _source_constants():
    """Every `constexpr int NAME = EXPR;` (and `#define NAME INT`) of the table's files, evaluated:
    EXPR is a product / sum of integers and earlier names."""
    text = {}
    for f in sorted({v[1] for v in se.CONSTANTS.values()}):
        with open(os.path.join(ROOT, f)) as fh:
            text[f] = fh.read()
    raw = {}
    for f, t in text.items():
        for name, val in re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)\s*$", t, re.M):
            raw.setdefault(name, val)
        for name, expr in re.findall(r"^\s*(?:static\s+)?constexpr\s+int\s+(\w+)\s*=\s*([^;]+);", t, re.M):
            raw.setdefault(name, expr)

    def value(name, depth=0):
        expr = raw[name]
        assert depth < 8 and re.fullmatch(r"[\w\s*+\-()]+", expr), (name, expr)
        return int(eval(re.sub(r"[A-Za-z_]\w*", lambda m: str(value(m.group(0), depth + 1)), expr)))  # noqa: S307

    out = {}
    for key, (_, f, sym) in se.CONSTANTS.items():
        if key == "KEY_PAD":    # keys_ld(K) { return (K + 31) & ~31; }
            m = re.search(r"int\s+keys_ld\(int K\)\s*\{\s*return\s*\(K \+ (\d+)\) & ~(\d+);", text[f])
            assert m and m.group(1) == m.group(2), "keys_ld changed its form: update shape_edges.CONSTANTS"
            out[key] = int(m.group(1)) + 1
        else:
            assert re.search(r"constexpr\s+int\s+" + sym + r"\b", text[f]), (sym, "not defined in", f)
            out[key] = value(sym)
    return out


def test_table_equals_the_sources():
    got = _source_constants()
    for key, (val, f, sym) in se.CONSTANTS.items():
        assert got[key] == val, (f"tests/shape_edges.py CONSTANTS[{key!r}] = {val}, but {f} has {sym} = "
                                 f"{got[key]}: update the table (its shapes follow) with the source")


def test_shapes_sit_on_the_edges():
    """The lists hold what the table's notes say, in numbers (config 4's K = 6 * 512 + 1 is one)."""
    Ks = [k for k, _ in se.K_EDGES]
    assert Ks[:9] == [63, 64, 65, 3072, 3073, 3074, 6144, 6145, 6146]
    # (one K edge serves the fused chain's reach and the 3-per-thread index's; fiw's threads are full)
    assert se.kIndexMaxK == se.kFwMaxK and se.kFwMaxK % se.kFwThreads == 0
    for K, r in zip(Ks[9:], (2, 3, 4)):
        assert 64 <= K < 256 and K % 6 == r and K % 8 and K % 16 and K % 32, K
    assert se.K_FOR_N == 70
    assert [n for n, _ in se.N_EDGES] == [1, 2, 7, 8, 9, 511, 512, 513, 2048, 2049]
    assert [n for n, _ in se.GEN_N] == [11, 14, 511, 512, 513, 516]
    assert se.SMALL_K == tuple(range(1, 37))
    flips = [K for K in se.SMALL_K[1:] if se.xk(K) != se.xk(K - 1)]
    # (prep_x_kernel from K = 6, 12, 18, 24, 30 on; prep_kernel again from 8, 15, 22, 29 on, where
    # K mod 6 exceeds K div 6; every K >= 30 takes prep_x_kernel)
    assert flips == [6, 8, 12, 15, 18, 22, 24, 29, 30] and all(se.xk(K) for K in range(30, 300)), flips
    # the generated-source layouts (eval_plan.h eval_plan: gen_x, pair)
    lay = [("gen_x" if N <= se.kPrepU else "pair" if (3 * N) % 4 == 0 else "chains") for N, _ in se.GEN_N]
    assert lay == ["gen_x"] * 4 + ["chains", "pair"]
    assert (3 * 14) % 4 != 0 and 6 * 513 > se.kFwMaxK + 1
    # routes (shape_edges.route): the fused chain's reach
    for K in (64, 65, 3072, 3073):
        assert se.route(8, K, chain="fused") == (True, True) == se.route(8, K, fresh=True)
        assert se.route(8, K, chain="five") == (True, False)
    for chain in ("auto", "fused", "five"):
        assert se.route(8, 63, chain=chain) == (False, False)
        assert se.route(8, 3074, chain=chain) == (True, False)
        assert se.route(8, 5, "poll", chain) == (True, chain == "fused" or (None if chain == "auto" else False))
    assert se.route(2048, 70, "tiled", "fused") == (True, False)
    assert se.route(2049, 70, "tiled", "fused") == (True, True)
    assert se.route(2049, 1, "auto", "fused") == (True, True)


# ---------------------------------------------------------------------------- the route plan

def _table_shapes():
    """(N, K) of every K_EDGES, SMALL_K and N_EDGES shape."""
    return ([(se.N_K, K) for K, _ in se.K_EDGES] + [(se.N_K, K) for K in se.SMALL_K]
            + [(N, se.K_FOR_N) for N, _ in se.N_EDGES])


def _ceil(a, b):
    return -(-a // b)


def test_plan_equals_the_table_for_matrix_polls():
    """eval_plan (through mac_diag_route) at every table shape under every algorithm and chain option:
    what the launch roles cannot show (the index's candidates per thread, the fused prep's kernel, the
    launch sizes) against the table's own arithmetic."""
    for N, K in _table_shapes():
        for algo in ("auto", "tiled", "poll"):
            for chain in ("auto", "fused", "five"):
                p = se.plan(N, K, algo, chain)
                tag = (N, K, algo, chain, vars(p))
                runs, fiw = se.route(N, K, algo, chain)
                assert bool(p.poll_possible) == runs, tag
                assert bool(p.fused_eligible) == (fiw is not False), tag
                iper = 3 if K <= se.kIndexMaxK + 1 else 6 if K <= se.kIndexMaxKWide + 1 else 0
                assert p.iper == iper and bool(p.want_keys) == (runs and iper != 0), tag
                assert p.nfw == p.nidx == se.WG_ALIGN * _ceil(N, se.WG_ALIGN), tag
                assert p.nfin2 == 8 * _ceil(K, 8 * se.kF2C), tag
                assert (p.pair, p.gen_x, p.mesh) == (0, 0, 0), tag
                assert p.nchain == _ceil(K, se.kPrepC), tag
                x = se.xk(K, N)
                assert p.prep_fused == (se.PREP_X_MATRIX if x else se.PREP_KERNEL), tag
                assert p.nprep == (K // se.kPrepCX if x else _ceil(K, se.kPrepC)), tag
                assert p.xbase == K // se.kPrepCX * se.kPrepCX, tag
                assert (p.prep_five, p.nrec) == (se.PREP_KERNEL, _ceil(K, se.kPrepC)), tag
                assert p.counts == (1 if runs else 0), tag
    assert [K for K in se.SMALL_K[1:]
            if se.plan(se.N_K, K, "poll").prep_fused != se.plan(se.N_K, K - 1, "poll").prep_fused] \
        == [6, 8, 12, 15, 18, 22, 24, 29, 30]
    assert [se.plan(se.N_K, K).iper for K in (3073, 3074, 6145, 6146)] == [3, 6, 6, 0]
    assert se.plan(se.N_K, 70, w_uniform=False).counts == 0


def test_plan_forces_the_walk_at_the_lds_limit():
    """algo="tiled" is honoured at N = kTiledMaxN and becomes the poll walk one disk above."""
    K = se.K_FOR_N
    poll, tiled = se.plan(8, K, "poll").walk_forced, se.plan(se.kTiledMaxN, K, "tiled").walk_forced
    assert poll != 0 and tiled != 0 and poll != tiled
    assert se.plan(se.kTiledMaxN, K, "auto").walk_forced == 0
    for algo in ("auto", "tiled", "poll"):
        assert se.plan(se.kTiledMaxN + 1, K, algo).walk_forced == poll, algo
        assert se.plan(se.kTiledMaxN + 1, 1, algo).poll_possible == 1, algo
    assert se.plan(se.kTiledMaxN, K, "tiled", "fused").fused_eligible == 0
    assert se.plan(se.kTiledMaxN + 1, K, "tiled", "fused").fused_eligible == 1


def test_plan_leaves_failures_out_of_the_walk_up_to_kPrepU():
    """excl: objectives-only requests with cons3 or a mask byte, N <= kPrepU."""
    for N, _ in se.N_EDGES:
        for want_area in (False, True):
            for want_obj in (False, True):
                for cons3 in (False, True):
                    for mask in (False, True):
                        p = se.plan(N, se.K_FOR_N, want_area=want_area, want_obj=want_obj, cons3=cons3, mask=mask)
                        want = want_obj and (cons3 or mask) and not want_area and N <= se.kPrepU
                        assert bool(p.excl) == want, (N, want_area, want_obj, cons3, mask)
    assert se.plan(se.kPrepU, se.K_FOR_N, cons3=True).excl == 1
    assert se.plan(se.kPrepU + 1, se.K_FOR_N, cons3=True).excl == 0


def test_plan_generated_layouts():
    """GEN_N as a generated source and in basis form (K = 6N at mesh step 8): gen_x up to kPrepU, then
    prep_kernel by candidates or by pairs; an xy-only poll (K = 4N) never takes gen_x; a step above 8
    keeps a poll the host can size out of the fused chain unless it is forced."""
    lay = ["gen_x", "gen_x", "gen_x", "gen_x", "chains", "pair"]
    for (N, _), want in zip(se.GEN_N, lay):
        K, n = 6 * N, 3 * N
        for kind in (se.SRC_GENERATED, se.SRC_BASIS):
            for chain in ("auto", "fused", "five"):
                p = se.plan(N, K, "auto", chain, kind=kind, b=2 ** se.ELL, delta=1.0, cons3=True)
                tag = (N, kind, chain, vars(p))
                assert (bool(p.gen_x), bool(p.pair and not p.gen_x)) == (want == "gen_x", want == "pair"), tag
                assert p.nchain == (n // 4 if (n % 4 == 0) else _ceil(K, se.kPrepC)), tag
                if want == "gen_x":
                    assert (p.prep_fused, p.nprep) == (se.PREP_X_GEN, N), tag
                    assert (p.prep_five, p.nrec) == (se.PREP_X_GEN, N), tag
                else:
                    assert (p.prep_fused, p.nprep) == (se.PREP_KERNEL, p.nchain), tag
                    assert (p.prep_five, p.nrec) == (se.PREP_KERNEL, p.nchain), tag
                assert bool(p.fused_eligible) == (chain != "five" and K <= se.kFwMaxK + 1), tag
                assert bool(p.excl) == (N <= se.kPrepU), tag
            # an xy-only poll of the same UAVs
            q = se.plan(N, 4 * N, kind=kind, np_=2 * N, b=2 ** se.ELL, delta=1.0)
            assert q.gen_x == 0 and bool(q.pair) == ((2 * N) % 4 == 0), (N, kind, vars(q))
            assert q.prep_fused == se.PREP_KERNEL and q.prep_five == se.PREP_KERNEL, (N, kind, vars(q))
    # the wide step, the host's crowding estimate and the pipelined loop's device-side step
    N0 = se.GEN_N[0][0]
    for kw in (dict(kind=se.SRC_GENERATED, b=16), dict(kind=se.SRC_BASIS, b=8, delta=1.5),
               dict(kind=se.SRC_GENERATED, b=8, route_five=True)):
        assert se.plan(N0, 6 * N0, **kw).fused_eligible == 0, kw
        assert se.plan(N0, 6 * N0, "auto", "fused", **kw).fused_eligible == 1, kw
    assert se.plan(N0, 6 * N0, kind=se.SRC_GENERATED, b=16, mst=True).fused_eligible == 1
    assert se.plan(N0, 6 * N0, kind=se.SRC_GENERATED, b=8, mesh=True).mesh == 1
    assert se.plan(N0, 6 * N0, kind=se.SRC_GENERATED, b=8, k0=1).gen_x == 0


# ---------------------------------------------------------------------------- the cases

def _cases():
    out = []
    for K, _ in se.K_EDGES:
        out += [(se.N_K, K, False, False), (se.N_K, K, False, True)]
        if K in se.K_WEIGHTED:
            out.append((se.N_K, K, True, False))
    for K in se.SMALL_K:
        out += [(se.N_K, K, False, False), (se.N_K, K, False, True)]
    for N, _ in se.N_EDGES:
        out += [(N, se.K_FOR_N, False, False), (N, se.K_FOR_N, False, True)]
        if N in se.N_WEIGHTED:
            out.append((N, se.K_FOR_N, True, False))
    return out


def _id(p):
    N, K, weighted, last = p
    return f"N{N}-K{K}" + ("-w" if weighted else "") + ("-last" if last else "")


def _exp(orc, p):
    if p not in _EXP:
        N, K, weighted, last = p
        c = se.make(N, K, weighted=weighted, argmin_last=last)
        _EXP[p] = (c, se.expected(orc, c))
    return _EXP[p]


def _np_weighted_area(c, k):
    """Row k's area on the lattice list from integer tests per disk window (numpy; the equivalence
    with sqrt(a) < r for integer disks: oracle.lattice_count)."""
    G, N = c.G, c.N
    v = c.C[k].astype(np.int64)
    cov = np.zeros((G, G), dtype=bool)
    for u in range(N):
        cx, cy, R = int(v[u]), int(v[N + u]), int(v[2 * N + u])
        if R <= 0:
            continue
        i0, i1 = max(1, (cx - R) // 5), min(G, (cx + R) // 5 + 2)
        j0, j1 = max(1, (cy - R) // 5), min(G, (cy + R) // 5 + 2)
        if i0 > i1 or j0 > j1:
            continue
        dx = ((2 * np.arange(i0, i1 + 1) - 1) * 5 - 2 * cx)[:, None]
        dy = ((2 * np.arange(j0, j1 + 1) - 1) * 5 - 2 * cy)[None, :]
        cov[i0 - 1:i1, j0 - 1:j1] |= (dx * dx + dy * dy) < 4 * R * R
    return float(c.w.reshape(G, G)[cov].sum())


@pytest.mark.parametrize("p", _cases(), ids=_id)
def test_case_has_teeth(orc, p):
    N, K, weighted, last = p
    c, e = _exp(orc, p)
    assert c.C.shape == (K, 3 * N) and c.x.size == c.G * c.G
    # on the mesh around candidate 0: packed keys, the direct-mapped table
    assert np.array_equal(c.C[0][None, :] + c.D, c.C) and np.abs(c.D).max(initial=0) <= 8
    assert np.array_equal(c.C, np.round(c.C)) and (c.C[:, 2 * N:] > 0).all()
    # two references agree
    if weighted:
        for k in range(K):
            assert e.area[k] == _np_weighted_area(c, k), k
    else:
        assert np.array_equal(e.area, 25.0 * orc.lattice_count_batch(c.C, c.G).astype(np.float64))
    # the areas differ, and the union stays far from the whole list
    assert np.unique(e.area).size >= min(8, K // 2), np.unique(e.area).size
    assert 0 < e.area.max() < 0.5 * c.w.sum()
    # the penalties differ: r_max lies inside the radius offsets' range, so the objective is not
    # -area; the rows at the end of the matrix's / a thread's reach carry one, and so does a UAV of
    # every block of the penalty chain (the last UAV among them)
    viol = orc.violation_batch(c.C, c.r_max)
    per_uav = np.abs(c.D[:, 2 * N:] - c.A[None, :])
    assert np.array_equal(viol, per_uav.sum(axis=1)) and np.array_equal(e.obj, -e.area + viol * 1e5)
    assert np.unique(viol).size >= min(4, K // 2), np.unique(viol)
    if last:
        assert K == 1 or (viol[K - 1] == 0 and (viol[:K - 1] > 0).all())
    else:
        if K >= 4:
            assert (viol == 0).any() and (viol > 0).any()
        assert K == 1 or viol[K - 1] > 0
        assert K <= se.kFwMaxK or viol[se.kFwMaxK] > 0
    if K >= 8:
        for b in range(0, N, se.kPrepU):
            assert np.unique(per_uav[:, b:b + se.kPrepU].sum(axis=1)).size >= 2, b
        assert np.unique(per_uav[:, N - 1]).size >= 2
    # cons3 splits the poll; the rows at the end of a thread's / the matrix's reach pass; the
    # first failing row fails through the last UAV alone (the last block's, N > kPrepU)
    nf = int(e.feas.sum())
    if K >= 8:
        assert 0 < nf < K, nf
        k = se.FAIL_EVERY // 2
        assert not e.feas[k] and abs(c.D[k, N - 1]) == se.FAIL_OFFSET == abs(c.D[k, 2 * N - 1])
        assert np.abs(c.D[k, :2 * N]).max(initial=0) == se.FAIL_OFFSET
        assert (np.abs(np.delete(c.D[k, :2 * N], [N - 1, 2 * N - 1])) <= se.OFFSET).all()
    assert e.feas[K - 1] and (K <= se.kFwMaxK or e.feas[se.kFwMaxK])
    # shared entries exist
    if N >= 2:
        one = [orc.np_covered(c.C[0][[u, N + u, 2 * N + u]], c.x, c.y) for u in (0, 1)]
        assert (one[0] & one[1]).any()
    if last:
        # the last row is the strict minimiser with and without cons3: a dropped last candidate
        # changes the argmin and the best objective
        assert e.k == K - 1 == e.k_bar
        if K > 1:
            assert e.obj[K - 1] < e.obj[:K - 1].min() and e.bar[K - 1] < e.bar[:K - 1].min()
    if K == se.kFwMaxK + 1:
        # candidate kFwMaxK (fiw_kernel's thread 0, its thirteenth) read as candidate 0 instead
        # changes the expected area and objective
        assert e.area[se.kFwMaxK] != e.area[0] and e.obj[se.kFwMaxK] != e.obj[0]


@pytest.mark.parametrize("N", [n for n, _ in se.GEN_N])
def test_generated_case_has_teeth(orc, N):
    """The basis-form polls: K = 6N rows on the mesh at step 8 with positive radii; cons3 splits them;
    the exact lattice count (the GPU test's reference at these sizes) equals the C oracle on a
    sample of rows (every row up to K = 256; the C oracle takes ~7 ms per row at N = 513)."""
    c = se.make_gen(N)
    K = c.K
    assert K == 6 * N and c.C.shape == (K, 3 * N)
    B = c.L[c.rp][:, c.cp]
    assert np.abs(B).max() == 2 ** se.ELL and np.array_equal(c.C[:3 * N], c.x0[None, :] + B.T)
    assert np.array_equal(c.C, np.round(c.C)) and (c.C[:, 2 * N:] > 0).all()
    e = se.expected(orc, c, exact=False)
    rows = np.arange(K) if K <= 256 else np.unique(np.concatenate([np.arange(0, K, 191), [K - 1]]))
    rec = np.stack([c.x, c.y, c.w, c.w, np.zeros_like(c.x)], axis=1)
    assert np.array_equal(orc.PointerList(rec).area_batch(c.C[rows]), e.area[rows])
    assert np.unique(e.area).size >= 8 and 0 < e.area.max() < 0.5 * c.w.sum()
    assert 0 < int(e.feas.sum()) < K
