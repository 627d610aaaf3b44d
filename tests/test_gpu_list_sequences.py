"""GPU: list maintenance against a host model (tests/list_cases.py Model and sequences; replayed on
the model alone by tests/test_list_cases.py).

Each sequence runs in a context of its own: set (every entry point), append (host and device; empty,
one entry, more than doubling the list, outside the bounding box, onto no list and onto an emptied
one), remove_covered (a 5-disk state, no disk, disks that cover nothing, r = inf, the same circles
twice), regions set and cleared in between. After every operation the device list equals the model
bit for bit, the per-entry flags of a probe state equal the oracle's, and one K = 67 poll, through a
path that rotates over auto, the five-launch chain, the fused chain and the per-candidate walk,
equals the oracle on the model; every fourth operation the attribution and, with regions on, the
ingest counts and the region stats are compared too. Weights are 25, or 100 inside the boxes: every
sum is exact and every comparison `==`.

The routing state that outlives a list change (the context's crowded-poll history, the lanes'
shared-entry hints) is exercised by `stale_route`: polls on a crowded list, then another list and
another poll on the same context, and back.

Expected values: src/CellFunctions.jl:81-108 (rmvCoveredPOI), :42-45 / :68-72 (the override),
src/AreaCoverageCalculation.jl:63-78 (calculateArea), all through the oracle and numpy.
"""
import numpy as np
import pytest
import torch

import list_cases as lc
from test_gpu_boundary import _profiled
from test_gpu_bydisk import np_by_disk
from test_gpu_regions import _assert_stats, _expect_stats

pytestmark = pytest.mark.gpu

PATHS = (("auto", "auto"), ("poll", "five"), ("poll", "fused"), ("tiled", "auto"))


def _dev(v):
    return torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, device=torch.device("cuda", 0))


def _apply(ctx, op):
    """One operation on the device list; returns the kept indices for a removal."""
    kind = op["op"]
    if kind in ("set", "append"):
        x, y, w = op["pts"]
        how = op["how"]
        if how == "set_points_records":
            ctx.set_points_records(lc.recs(x, y, w))
        elif how in ("set_points_device", "append_points_device"):
            t = [_dev(v) for v in (x, y, w)]
            getattr(ctx, how)(*t)
            torch.cuda.synchronize()
        else:
            getattr(ctx, how)(x, y, w)
    elif kind == "remove":
        return ctx.remove_covered(op["circles"])
    elif kind == "regions":
        ctx.set_regions(*op["boxes"], w_high=op["w_high"])
    elif kind == "clear_regions":
        ctx.clear_regions()
    return None


def _want_area(orc, model, C):
    if model.x.size == 0:
        return np.zeros(C.shape[0])
    return orc.PointerList(lc.recs(model.x, model.y, model.w)).area_batch(C)


def _poll(ctx, orc, model, C, path, where):
    ctx.set_algo(path[0])
    ctx.set_chain(path[1])
    got = ctx.area_batch(C)
    want = _want_area(orc, model, C)
    bad = np.flatnonzero(got != want)
    if bad.size:
        cand = C[int(bad[0])]
        flags, wf = ctx.covered_flags(cand), orc.np_covered(cand, model.x, model.y)
        e = np.flatnonzero(flags != wf)[:8]
        raise AssertionError((where, path, bad[:8], got[bad[:8]], want[bad[:8]],
                              [(int(i), float(model.x[i]), float(model.y[i]), bool(wf[i])) for i in e]))


@pytest.mark.parametrize("name", lc.SEQUENCES)
def test_sequence(pkg, orc, name):
    ops = lc.make_sequence(name)
    model = lc.Model(orc)
    turn = 0
    with pkg.Context(0) as ctx:
        for q, op in enumerate(ops):
            where = (name, q, op["op"], op.get("how"))
            kept = _apply(ctx, op)
            want_kept = lc.apply_to_model(model, op)
            if op["op"] == "remove":
                assert np.array_equal(kept, want_kept), (where, kept.size, want_kept.size)
            if not model.has_list:        # (regions set before the first list: nothing to read yet)
                continue
            assert ctx.num_points == model.x.size, where
            gx, gy, gw = ctx.get_points()
            assert gx.tobytes() == model.x.tobytes() and gy.tobytes() == model.y.tobytes(), where
            assert gw.tobytes() == model.w.tobytes(), where
            probe, C = op["probe"], op["C"]
            flags = ctx.covered_flags(probe)
            want_flags = orc.np_covered(probe, model.x, model.y)
            assert np.array_equal(flags, want_flags), (where, np.flatnonzero(flags != want_flags)[:8])
            if op["op"] == "polls":
                paths = op.get("paths", (PATHS[0],))

                def polls():
                    for i in range(op["n"]):
                        _poll(ctx, orc, model, C, paths[i % len(paths)], where + (i,))

                _, kern = _profiled(ctx, polls)
                print(f"{where}: {kern}")
                if op.get("expect_shared"):
                    # the lanes take turns and the pass is launched on a lane's own earlier polls:
                    # over the run of crowded polls it must have run, or no routing state is stale
                    assert kern.get("shared_or_kernel", 0) > 0, (where, kern)
            _poll(ctx, orc, model, C, PATHS[turn % len(PATHS)], where)
            turn += 1
            if q % 4 == 3:
                ctx.set_algo("auto")
                ctx.set_chain("auto")
                owned, excl, area = ctx.area_by_disk(probe)
                wo, wx, wa = np_by_disk(orc, probe, model.x, model.y, model.w)
                assert np.array_equal(owned, wo) and np.array_equal(excl, wx) and area == wa, where
                if model.boxes is not None:
                    cnt, tot = ctx.regions_ingested()
                    assert np.array_equal(cnt, model.cnt) and tot == model.tot, where
                    if model.x.size:
                        _assert_stats(ctx.region_stats(probe),
                                      _expect_stats(model.x, model.y, model.w, model.boxes, probe, orc),
                                      where=str(where))
