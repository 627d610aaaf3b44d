"""GPU: fin2_kernel's shared-entry pass (k_fiw.h): the disks with lower-index neighbours hand their
shared entries to the finalize launch, which decides them per candidate. The smallest layouts at
which that pass can go wrong, each through the forced fused chain: every area against the C oracle's
first-hit sum (src/AreaCoverageCalculation.jl:63-78), every objective against the reference
objective (src/TDM_STATIC_opt.jl:82-100; +inf for a candidate failing cons3,
src/TDM_Constraints.jl:54-75), and (area, objective, argmin) against the five-launch chain on the
same inputs. The layouts are in fin2_layouts.py."""
import numpy as np
import pytest

from fin2_layouts import TAN50, geometry
from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
_REF = {}


def _reference(case, pkg, orc):
    """(points, candidates, r_max, d_lim, areas, objectives, cons3 feasibility) of a case: computed once,
    shared by the tests and never modified."""
    if case not in _REF:
        _, (x, y, w), C, rmax, dlim = geometry(case, pkg.workloads)
        rec = recs(x, y, w)
        area = orc.PointerList(rec).area_batch(C)
        obj = np.array([orc.ref_objective(c, rec, rmax) for c in C])
        feas = orc.cons3_batch(C[0], C, dlim, TAN50)
        for a in (C, rmax, dlim, area, obj, feas, x, y, w):
            a.setflags(write=False)
        _REF[case] = ((x, y, w), C, rmax, dlim, area, obj, feas)
    return _REF[case]


def _run(ctx, chain, C, rmax, dlim, cons3):
    """(areas, objectives, best objective, argmin, launches by kernel) through a forced chain."""
    ctx.set_chain(chain)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    area = ctx.area_batch(C)
    if cons3:
        bo, bi, objs = ctx.poll_best(C, rmax, 1e5, prev=C[0], d_lim=dlim,
                                     tan_half_fov=TAN50, want_all=True)
    else:
        bo, bi, objs = ctx.poll_best(C, rmax, 1e5, want_all=True)
    kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    ctx.profile_read(reset=True)
    ctx.profile(False)
    return area, objs, bo, bi, kern


def _check(ctx, pkg, orc, case, cons3):
    (x, y, w), C, rmax, dlim, want_area, want_obj, feas = _reference(case, pkg, orc)
    ctx.set_points(x, y, w)
    want = np.where(feas, want_obj, np.inf) if cons3 else want_obj
    try:
        fa, fo, fbo, fbi, kern = _run(ctx, "fused", C, rmax, dlim, cons3)
        va, vo, vbo, vbi, _ = _run(ctx, "five", C, rmax, dlim, cons3)
    finally:
        ctx.set_chain("auto")
        ctx.profile(False)
    assert kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern
    bad = np.flatnonzero(~((fa == want_area) | (np.isnan(fa) & np.isnan(want_area))))
    assert bad.size == 0, (case, bad[:5], fa[bad[:5]], want_area[bad[:5]])
    assert np.array_equal(fo, want, equal_nan=True), (case, np.flatnonzero(fo != want)[:5])
    assert np.array_equal(fa, va, equal_nan=True), case
    assert np.array_equal(fo, vo, equal_nan=True), case
    assert fbi == vbi and (fbo == vbo or (np.isnan(fbo) and np.isnan(vbo))), (case, fbi, vbi, fbo, vbo)
    return C, feas


@pytest.mark.parametrize("cons3", [False, True])
def test_pairs_partial_last_block(ctx, pkg, orc, cons3):
    """N = 12 in six pairs 10 m apart (six listed disks, one lower neighbour each: the bench
    workload's situation), K = 73: the last finalize block holds 9 of its 16 candidates."""
    C, _ = _check(ctx, pkg, orc, "pairs", cons3)
    assert C.shape[0] == 73 and C.shape[0] % 16 == 9


@pytest.mark.parametrize("cons3", [False, True])
def test_up_to_four_neighbours(ctx, pkg, orc, cons3):
    """N = 13: two clusters of 5 mutually overlapping disks (1, 2, 3 and 4 lower neighbours, the
    most a listed disk carries) and 3 disks on their own."""
    _check(ctx, pkg, orc, "four_neighbours", cons3)


@pytest.mark.parametrize("cons3", [False, True])
def test_several_chunks(ctx, pkg, orc, cons3):
    """N = 24 in twelve pairs: more handed-off entries than one staged chunk holds (2048), each
    disk under the per-disk cap."""
    _check(ctx, pkg, orc, "chunks", cons3)


@pytest.mark.parametrize("cons3", [False, True])
def test_weighted_list(ctx, pkg, orc, cons3):
    """The pairs under weights from {25, 50, 75}: the fp64-credit build, whose sums keep the
    sorted list's order; equal to the oracle and to the five-launch chain bit for bit."""
    (x, y, w), *_ = _reference("weighted", pkg, orc)
    assert np.unique(w).size == 3
    _check(ctx, pkg, orc, "weighted", cons3)


@pytest.mark.parametrize("cons3", [True, False])
def test_dead_and_nonfinite_candidates(ctx, pkg, orc, cons3):
    """The pairs under an ell = 3 poll with a NaN radius and a radius <= 0 on listed disks, about
    half of the candidates failing cons3 (35 of 73 at d_lim = 9 m; at N = 12 the usual 10 m fails
    only 11): those are skipped in the shared pass, their neighbours in the block are not."""
    C, feas = _check(ctx, pkg, orc, "dead_nonfinite", cons3)
    K = C.shape[0]
    dead = np.flatnonzero(~feas)
    assert K // 3 <= dead.size <= 2 * K // 3, dead.size   # (about half)
    assert np.unique(dead // 16).size == (K + 15) // 16   # (dead and live in every finalize block)


@pytest.mark.parametrize("cons3", [False, True])
@pytest.mark.parametrize("case", ["batches", "batches_weighted"])
def test_two_batches_of_disk_records(ctx, pkg, orc, case, cons3):
    """N = 70 in 35 pairs: 70 disk records, more than one batch of the shared pass holds (64), so
    the second batch's slot owners, records and entries replace the first's; with equal weights and
    with weights from {25, 50, 75} (the fp64 build, its list sorted by disk)."""
    _check(ctx, pkg, orc, case, cons3)
