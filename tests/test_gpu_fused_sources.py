"""GPU: the fused chain's two source instantiations (k_fiw.h kMat). fiw_kernel and fin2_kernel are
built once for a matrix source and once for a generated one, so the two can drift apart: every case
here puts THE SAME poll through both,
  * as a matrix, Cm = [x0 + delta B^T; x0 - delta B^T] (B = L[rp][:, cp], workloads.
    ltmads_basis_parts), through poll_best from host memory and from device memory, and
  * in basis form (poll_basis: the generated source, expanded on the device),
each with the chain forced to "fused" and then to "five". Every (objective, index) pair and every
objective must be equal across all of them and equal to the C oracle's (the first-hit area,
src/AreaCoverageCalculation.jl:63-78; the objective, src/TDM_STATIC_opt.jl:82-100; +inf for a
candidate failing cons3, src/TDM_Constraints.jl:54-75), and the profile must show fiw_kernel and
fin2_kernel where the fused chain was forced. All comparisons are exact.

The poll has 2n = 6N = 72 candidates (N = 12 on grid_points(200)): the basis form carries no
incumbent row. The matrix with the incumbent in front (K = 6N + 1 = 73) goes through both chains as
well; its rows 1.. are the same poll."""
import math

import numpy as np
import pytest

from test_gpu_parity import recs
from test_gpu_parity import test_native_mads_pipelined_matches_stepper as _pipelined

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
G, N, R = 200, 12, 36.0
CASES = ("ell2", "ell3", "ell4", "escape", "weighted", "handoff", "inplace", "dead_slot")
_REF = {}


def _layout(case, wl, rng):
    """[x; y; r] of the incumbent: integer centres, the lattice's 1000 m square."""
    if case == "handoff":
        # two clusters of 5 mutually overlapping disks (1, 2, 3 and 4 lower neighbours: the most a
        # listed disk carries, kFwHand) and 2 disks on their own
        off = [(0, 0), (6, 0), (0, 6), (6, 6), (3, 3)]
        cx = [300.0 + a for a, b in off] + [700.0 + a for a, b in off] + [300.0, 700.0]
        cy = [300.0 + b for a, b in off] + [700.0 + b for a, b in off] + [700.0, 300.0]
        return np.concatenate([cx, cy, np.full(N, R)])
    if case == "inplace":
        # one cluster of 7 mutually overlapping disks (the last three: 4, 5 and 6 lower neighbours,
        # 5 and 6 past kFwHand: decided in place) and 5 disks on their own
        off = [(0, 0), (6, 0), (0, 6), (6, 6), (3, 3), (9, 3), (3, 9)]
        cx = [500.0 + a for a, b in off] + [150.0, 850.0, 150.0, 850.0, 500.0]
        cy = [500.0 + b for a, b in off] + [150.0, 150.0, 850.0, 850.0, 150.0]
        return np.concatenate([cx, cy, np.full(N, R)])
    x0 = wl.uniform_disks(N, G, rng)
    if case == "dead_slot":
        x0[2 * N + 3] = 4.0   # (ell = 2: its diagonal step of 4 takes one candidate's radius to 0)
    return x0


def _reference(case, pkg, orc):
    """A case's points, poll (basis parts and matrix), r_max, cons3 limit, and the oracle's
    objectives and feasibility: computed once, shared by both cons3 settings and never modified."""
    if case in _REF:
        return _REF[case]
    wl = pkg.workloads
    rng = wl.SplitMix64(7300 + CASES.index(case))
    x, y, w = wl.grid_points(G)
    if case == "weighted":   # two distinct weights: the fp64-credit builds
        w = np.where(rng.uniform(w.size) < 0.5, 25.0, 50.0)
        assert np.unique(w).size == 2
    x0 = _layout(case, wl, rng)
    n = 3 * N
    ell = {"ell3": 3, "ell4": 4}.get(case, 2)
    Lm, rp, cp = wl.ltmads_basis_parts(n, ell, rng)
    delta = 1.0
    if case == "escape":
        # the same integer steps as 0.5 x (2 L), then one entry of 2 L made odd: the two candidates
        # of that column move one variable by a half-integer, which no packed key holds (k_prep.h
        # "Packed keys": the key escapes and its disk takes one position per candidate)
        Lm = 2 * Lm
        delta = 0.5
        c = int(cp[5])
        c = c if c < n - 1 else int(cp[6])
        Lm[c + 1, c] += 1
    B = Lm[rp][:, cp].astype(np.float64)
    Cm = np.ascontiguousarray(np.concatenate([x0[None, :] + delta * B.T, x0[None, :] - delta * B.T]))
    K = Cm.shape[0]
    assert K == 6 * N and K >= 64
    if case == "escape":
        frac = Cm != np.floor(Cm)
        assert frac.sum() == 2 and not frac[0].any()
    if case == "dead_slot":
        assert int((Cm[:, 2 * N:] <= 0.0).sum()) == 1
    rmax = np.full(N, 30.0 * TAN50)
    # cons3's limit: the median over the candidates of their largest UAV move, so about half fail
    d = Cm.reshape(K, 3, N) - x0.reshape(1, 3, N)
    move = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + (d[:, 2] / TAN50) ** 2).max(axis=1)
    dlim = np.full(N, float(np.median(move)))
    rec = recs(x, y, w)
    C73 = np.ascontiguousarray(np.concatenate([x0[None, :], Cm]))
    obj = np.array([orc.ref_objective(c, rec, rmax) for c in C73])
    assert np.array_equal(obj, -orc.PointerList(rec).area_batch(C73) + orc.violation_batch(C73, rmax) * 1e5)
    feas = orc.cons3_batch(x0, C73, dlim, TAN50)
    assert feas[0] and 0 < int(feas[1:].sum()) < K, int(feas.sum())
    out = dict(x=x, y=y, w=w, x0=x0, Lm=Lm, rp=rp, cp=cp, delta=delta, Cm=Cm, C73=C73, rmax=rmax,
               dlim=dlim, obj=obj, feas=feas)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _REF[case] = out
    return out


def _dev_poll(ctx, C, rmax, prev, dlim):
    """poll_best from device memory: (best objective, index, objectives)."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)   # noqa: E731  (a writable copy)
    dC, dR = up(C), up(rmax)
    dB = torch.empty(2, dtype=torch.float64, device=dev)
    dO = torch.empty(C.shape[0], dtype=torch.float64, device=dev)
    kw = dict(d_prev=up(prev), d_dlim=up(dlim), tan_half_fov=TAN50) if prev is not None else {}
    ctx.poll_best_dev(dC, C.shape[1], C.shape[0], dR, dB, 1e5, d_obj=dO, **kw)
    torch.cuda.synchronize()
    bo, bi = ctx.best_fetch(dB)
    return bo, int(bi), dO.cpu().numpy()


def _profiled(ctx, fn):
    ctx.profile(True)
    ctx.profile_read(reset=True)
    out = fn()
    kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    ctx.profile_read(reset=True)
    ctx.profile(False)
    return out, kern


@pytest.mark.parametrize("cons3", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_same_poll_through_both_sources(ctx, pkg, orc, case, cons3):
    """ell2 / ell3: the direct-mapped table (9^3 and 17^3 slots); ell4: 33^3 slots exceed it, the
    hash; escape: one half-integer step (an escaped key: one position per candidate, the candidates'
    own values read from the source); weighted: the fp64-credit builds; handoff: disks with 1-4 lower
    neighbours (the list fin2_kernel takes); inplace: disks with 5 and 6 (decided in fiw_kernel);
    dead_slot: one candidate with r <= 0. cons3: about half the candidates fail (the dead word, the
    inert position)."""
    r = _reference(case, pkg, orc)
    ctx.set_points(r["x"], r["y"], r["w"])
    want73 = np.where(r["feas"], r["obj"], np.inf) if cons3 else r["obj"]
    want = want73[1:]
    k = int(np.argmin(want))
    k73 = int(np.argmin(want73))
    prev, dlim = (r["x0"], r["dlim"]) if cons3 else (None, None)
    kw = dict(prev=prev, d_lim=dlim, tan_half_fov=TAN50) if cons3 else {}
    try:
        for chain in ("fused", "five"):
            ctx.set_chain(chain)
            runs = {
                "matrix/host": lambda: ctx.poll_best(r["Cm"], r["rmax"], 1e5, want_all=True, **kw),
                "matrix/device": lambda: _dev_poll(ctx, r["Cm"], r["rmax"], prev, dlim),
                "basis": lambda: ctx.poll_basis(r["x0"], r["Lm"], r["rp"], r["cp"], r["delta"], r["rmax"],
                                                1e5, want_all=True, **kw),
            }
            for tag, fn in runs.items():
                (bo, bi, objs), kern = _profiled(ctx, fn)
                bad = np.flatnonzero(objs != want)
                assert bad.size == 0, (case, cons3, chain, tag, bad[:8], objs[bad[:8]], want[bad[:8]])
                assert (bi, bo) == (k, want[k]), (case, cons3, chain, tag, bi, k, bo, want[k])
                if chain == "fused":
                    assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, (tag, kern)
                else:
                    assert "fiw_kernel" not in kern and "fin2_kernel" not in kern, (tag, kern)
            # the incumbent in front (K = 6N + 1): rows 1.. are the same poll
            bo, bi, objs = ctx.poll_best(r["C73"], r["rmax"], 1e5, want_all=True, **kw)
            assert np.array_equal(objs, want73), (case, cons3, chain, np.flatnonzero(objs != want73)[:8])
            assert (bi, bo) == (k73, want73[k73]), (case, cons3, chain, bi, k73)
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)


def test_native_mads_takes_the_generated_instantiation(ctx, pkg):
    """mac_mads_run on a uniform layout with the fused chain forced == the stepper (a few polls,
    generated candidates, cons3): those calls still get the generated instantiation, and the
    profile shows the fused launches ran."""
    ctx.set_chain("fused")
    try:
        _, kern = _profiled(ctx, lambda: _pipelined(ctx, pkg, 40, 6, 2, 5, True, False))
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)
    assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern
