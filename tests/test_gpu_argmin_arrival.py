"""GPU: the poll argmin's two-level arrival (k_final.h finalize_argmin: block b adds to shard word
b & 7, the block that completes a shard adds to the root word, the block that completes the root
reduces the published minima and resets all nine words), through fin2_kernel (the fused chain) and
finalize_kernel (the five-launch chain).

Every poll is checked three ways: its objectives against the C oracle (exact), its (objective, index)
against numpy's first minimum of the objectives the same call returned, and against the candidate
the poll was built to prefer.

Shapes: N = 8 disks of radius 20 on a 64 x 64 lattice at 5 m, far enough apart not to overlap. Every
candidate shrinks one radius by 1..3 (so it covers strictly less) except the chosen ones, which
shrink none: the minimum is where the test puts it, and the other candidates tie in threes.

  * candidate blocks of 16: 1, 2, 7, 8, 9, 15, 16 and 17 of them (K = 16 x blocks) and K = 250 (a
    last block of 10). Both launches round their grid up to a multiple of 8 blocks; the blocks past
    K publish (+inf, -1) and take part in the arrival only, so these K give grids of 8, 16 and 24
    blocks with 1..17 of them holding candidates. The fused chain takes K >= 64, so K = 16 and 32 go
    through the five-launch chain alone.
  * K = 4112 (five-launch): 264 blocks, past the kFinMaxBlk = 256 minima the reducer loads at once.
  * the minimum in each of the 8 shards in turn (K = 256: 16 blocks, candidate block c runs as block
    (c % 2) * 8 + c / 2, shard c / 2).
  * an exact tie between blocks of different shards: the lowest index wins.
  * every candidate failing cons3: (+inf, -1).
  * polls of different K in a row on one stream (shards of 3, 1 and 2 blocks): the words reset."""
import math

import numpy as np
import pytest

from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
N, G = 8, 64
BLOCKS = (1, 2, 7, 8, 9, 15, 16, 17)
KS = tuple(16 * b for b in BLOCKS) + (250,)
_REF = {}
_LIST = {}


def _points(pkg):
    if not _LIST:
        x, y, w = pkg.workloads.grid_points(G)
        _LIST.update(x=x, y=y, w=w, rec=recs(x, y, w), rmax=np.full(N, 30.0 * TAN50))
    return _LIST


def _x0():
    cx = np.array([60.0, 160.0, 260.0, 60.0, 160.0, 260.0, 60.0, 160.0])
    cy = np.array([60.0, 60.0, 60.0, 160.0, 160.0, 160.0, 260.0, 260.0])
    return np.concatenate([cx, cy, np.full(N, 20.0)])


def _poll(K, best):
    """K candidates: candidate k shrinks disk k % N by 1 + (k / N) % 3, those in `best` none."""
    C = np.repeat(_x0()[None, :], K, axis=0)
    k = np.arange(K)
    C[k, 2 * N + k % N] -= 1.0 + (k // N) % 3
    for b in best:
        C[b] = _x0()
    return np.ascontiguousarray(C)


def _reference(pkg, orc, K, best):
    """The poll and the oracle's objectives: computed once per (K, best), read-only."""
    key = (K, tuple(best))
    if key not in _REF:
        p = _points(pkg)
        C = _poll(K, best)
        obj = -orc.PointerList(p["rec"]).area_batch(C) + orc.violation_batch(C, p["rmax"]) * 1e5
        assert int(np.argmin(obj)) == min(best) and int((obj == obj.min()).sum()) == len(best)
        C.setflags(write=False)
        obj.setflags(write=False)
        _REF[key] = (C, obj)
    return _REF[key]


def _check(ctx, pkg, orc, K, best, chain, **kw):
    p = _points(pkg)
    C, want = _reference(pkg, orc, K, best)
    ctx.profile(True)
    ctx.profile_read(reset=True)
    bo, bi, objs = ctx.poll_best(C, p["rmax"], 1e5, want_all=True, **kw)
    kern = {k: n for k, (ms, n) in ctx.profile_kernels().items() if n}
    ctx.profile_read(reset=True)
    ctx.profile(False)
    assert ("fin2_kernel" in kern) == (chain == "fused"), (chain, K, kern)
    assert np.array_equal(objs, want), (chain, K, np.flatnonzero(objs != want)[:8])
    k = int(np.argmin(objs))   # (numpy's: the first of equal minima)
    assert (bi, bo) == (k, objs[k]), (chain, K, bi, bo, k, objs[k])
    assert bi == min(best), (chain, K, bi, best)


@pytest.fixture
def chained(ctx, pkg):
    p = _points(pkg)
    ctx.set_points(p["x"], p["y"], p["w"])

    def use(chain):
        ctx.set_chain(chain)
        return ctx
    yield use
    ctx.set_chain("auto")
    ctx.profile(False)


@pytest.mark.parametrize("K,chain", [(K, ch) for K in KS for ch in ("fused", "five") if ch == "five" or K >= 64])
def test_blocks(chained, pkg, orc, K, chain):
    c = chained(chain)
    _check(c, pkg, orc, K, ((7 * K) // 11,), chain)
    _check(c, pkg, orc, K, (K - 1,), chain)   # the last candidate of the last block that holds any


def test_past_one_batch(chained, pkg, orc):
    K = 4112
    assert 8 * ((K + 127) // 128) > 256
    c = chained("five")
    _check(c, pkg, orc, K, (4100,), "five")   # block 256 of 264: past the reducer's first batch
    _check(c, pkg, orc, K, (3,), "five")


@pytest.mark.parametrize("chain", ["fused", "five"])
@pytest.mark.parametrize("shard", range(8))
def test_minimum_in_each_shard(chained, pkg, orc, shard, chain):
    c = chained(chain)
    _check(c, pkg, orc, 256, (32 * shard + 5,), chain)
    _check(c, pkg, orc, 256, (32 * shard + 16 + 11,), chain)   # the shard's other block


@pytest.mark.parametrize("chain", ["fused", "five"])
def test_tie_across_shards(chained, pkg, orc, chain):
    c = chained(chain)
    _check(c, pkg, orc, 256, (37, 200), chain)         # shards 1 and 6
    _check(c, pkg, orc, 256, (15, 16, 255), chain)     # the two blocks of shard 0, and shard 7
    _check(c, pkg, orc, 272, (130, 131, 260), chain)   # 24 blocks: shards of 3


@pytest.mark.parametrize("chain", ["fused", "five"])
def test_all_fail_cons3(chained, pkg, orc, chain):
    p = _points(pkg)
    C, _ = _reference(pkg, orc, 144, (77,))
    prev = C[0].copy()
    prev[:N] += 10.0
    dlim = np.full(N, 0.5)
    assert not orc.cons3_batch(prev, C, dlim, TAN50).any()
    c = chained(chain)
    bo, bi, objs = c.poll_best(C, p["rmax"], 1e5, prev=prev, d_lim=dlim, tan_half_fov=TAN50, want_all=True)
    assert (bo, bi) == (math.inf, -1) and np.all(objs == math.inf), (chain, bo, bi)
    _check(c, pkg, orc, 144, (77,), chain)   # and the words were reset by that poll's reducer


@pytest.mark.parametrize("chain", ["fused", "five"])
def test_polls_in_a_row(chained, pkg, orc, chain):
    c = chained(chain)
    for K in (272, 128, 250, 272, 250, 128):   # grids of 24, 8 and 16 blocks: shards of 3, 1 and 2
        _check(c, pkg, orc, K, ((5 * K) // 7,), chain)
