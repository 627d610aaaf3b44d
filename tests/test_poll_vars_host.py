"""CPU: the xy-only poll (MAC_POLL_XY, include/maxcover.h; the reference's CustomPoll,
src/TDM_STATIC_opt.jl:15-44) on the host mirrors alone. TDM_STATIC_opt.mads(poll_vars="xy") runs the
reference's per-trial-point loop on the C oracle (a plain-callable objective, cons1 and cons3 per
candidate): the fixture of test_native_mads_matches_oracle_loop, grid_points(160), N = 12, start
SplitMix64(2024), r_max = 30 tan 50 deg, d_lim = 10, N_iter = 30, ell0 = 2, ell_max = 5. With the
radii in place (36, 0.25 above r_max's granular best) the xy poll gains more area from fewer
evaluations; with the radii off (30) only the full poll can repair them."""
import math
import threading
from importlib import import_module

import numpy as np
import pytest

TAN50 = math.tan(100 / 180 * math.pi / 2)
N = 12
KW = dict(N_iter=30, ell0=2, ell_max=5)
_cache = {}


def _fixture(pkg, radii):
    wl = pkg.workloads
    x, y, w = wl.grid_points(160)
    rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
    rng = wl.SplitMix64(2024)
    x0 = np.concatenate([np.round(320 + rng.uniform(N) * 160), np.round(320 + rng.uniform(N) * 160),
                         np.full(N, radii)])
    return rec, x0, np.full(N, 30.0 * TAN50)


def _run(pkg, orc, radii, seed, poll_vars):
    """(x0, f(x0), x_out, f(x_out), objective evaluations of the polls), computed once."""
    key = (radii, seed, poll_vars)
    if key not in _cache:
        TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
        rec, x0, r_max = _fixture(pkg, radii)
        c3 = TC.create_cons3(x0, 100 / 180 * math.pi, np.full(N, 10.0))
        calls = [0]

        def objective(v):
            calls[0] += 1
            return orc.ref_objective(v, rec, r_max, 1e5)

        f0 = objective(x0)
        calls[0] = 0
        res = TS.mads(x0, objective, [TC.cons1, c3], seed=seed, poll_vars=poll_vars, **KW)
        assert res.x is not None and res.status.function_evaluations == calls[0]
        _cache[key] = (x0, f0, res.x, res.x_cost, calls[0] - 1, res)   # (- 1: f(x0))
    return _cache[key]


def test_radii_in_place_the_xy_poll_gains_more_from_fewer_evaluations(pkg, orc):
    x0, f0, x_xyr, f_xyr, ev_xyr, _ = _run(pkg, orc, 36.0, 99, "xyr")
    _, _, x_xy, f_xy, ev_xy, _ = _run(pkg, orc, 36.0, 99, "xy")
    assert x_xy[2 * N:].tobytes() == x0[2 * N:].tobytes()     # the radii: bit for bit
    assert x_xyr[2 * N:].tobytes() == x0[2 * N:].tobytes()    # (the full poll never won through one)
    assert f_xy < f_xyr < f0
    print(f"gain xy {f0 - f_xy!r} ({ev_xy} evaluations), xyr {f0 - f_xyr!r} ({ev_xyr})")
    assert f0 - f_xy == 3675.0 and f0 - f_xyr == 2625.0
    assert ev_xy == 232 and ev_xyr == 1089
    assert not np.array_equal(x_xy[:2 * N], x0[:2 * N])


def test_second_seed(pkg, orc):
    x0, f0, x_xyr, f_xyr, ev_xyr, _ = _run(pkg, orc, 36.0, 7, "xyr")
    _, _, x_xy, f_xy, ev_xy, _ = _run(pkg, orc, 36.0, 7, "xy")
    assert x_xy[2 * N:].tobytes() == x0[2 * N:].tobytes()
    assert f_xy < f_xyr < f0
    assert f0 - f_xy == 3850.0 and f0 - f_xyr == 2825.0
    assert ev_xy == 293 and ev_xyr == 916


def test_radii_off_the_full_poll_is_needed(pkg, orc):
    x0, f0, x_xyr, f_xyr, ev_xyr, _ = _run(pkg, orc, 30.0, 99, "xyr")
    _, _, x_xy, f_xy, ev_xy, _ = _run(pkg, orc, 30.0, 99, "xy")
    assert np.all(x_xyr[2 * N:] != x0[2 * N:])               # every radius moved
    assert x_xy[2 * N:].tobytes() == x0[2 * N:].tobytes()
    assert f0 - f_xy == 3075.0 and ev_xy == 369 and ev_xyr == 233
    # the xy poll cannot touch the 1e5 |R - r_max| charge (12 x 5.75 x 1e5 at x0): far above
    assert f_xyr < f_xy - 4e6
    assert f0 - f_xyr == pytest.approx(4756689.67, abs=0.01)


def test_candidates_of_an_xy_poll(pkg):
    """2 n_p candidates split at n_p, the basis on the first 2N variables, the radii copied (a -0.0
    radius stays -0.0: no r + 0.0), and the stream advancing by PollStepper._draws(n_p)."""
    TS, wl = pkg.TDM_STATIC_opt, pkg.workloads
    x = np.array([10.0, 20.0, 30.0, 40.0, 5.0, 6.0, -0.0, 7.5, 35.75])
    n_p = TS.polled_count(x.size, "xy")
    assert n_p == 6
    rng = wl.SplitMix64(5)
    B = wl.ltmads_basis(n_p, 3, rng).astype(np.float64)
    X = TS.poll_matrix(x, B)
    assert X.shape == (12, 9)
    assert np.array_equal(X[:6, :6], x[None, :6] + B.T) and np.array_equal(X[6:, :6], x[None, :6] - B.T)
    for row in X:
        assert row[6:].tobytes() == x[6:].tobytes()
    st = TS.PollStepper(x, 0.0, lambda Xs: (np.inf, -1), seed=5, poll_vars="xy")
    assert st.n == 6 and (st.lo, st.hi) == (0, 12) and st._draws() == 6 + 15 + 12
    r2 = wl.SplitMix64(5)
    r2.next_u64(st._draws())
    assert rng.state == r2.state
    # the full poll is what it was
    Bf = wl.ltmads_basis(9, 2, wl.SplitMix64(5)).astype(np.float64)
    assert np.array_equal(TS.poll_matrix(x, Bf), np.concatenate([x[None] + Bf.T, x[None] - Bf.T]))


class _ThreadGather:
    """An in-process exchange among `world` loops running on threads: every rank deposits its
    record, all wait, every rank reads all (what the all-gather computes)."""

    def __init__(self, world, combine):
        self.world, self.combine = world, combine
        self.slots = [None] * world
        self.barrier = threading.Barrier(world)

    def rank_view(self, rank):
        g = self

        class View:
            world = g.world

            def __init__(self):
                self.rank = rank

            def __call__(self, *rec):
                g.slots[rank] = rec
                g.barrier.wait()
                out = g.combine(list(g.slots))
                g.barrier.wait()
                return out

        return View()


def _threads(world, body):
    out, err = [None] * world, []

    def run(r):
        try:
            out[r] = body(r)
        except BaseException as e:   # noqa: BLE001 (reported below; the others' barrier is broken)
            err.append(e)
            raise

    ts = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not err, err
    return out


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("mode", ["sharded", "speculative"])
def test_poll_stepper_loops_end_on_mads_iterate(pkg, orc, world, mode):
    d = import_module(pkg.__name__ + ".dist")
    TS, TC = pkg.TDM_STATIC_opt, pkg.TDM_Constraints
    x0, f0, want_x, want_f, ev, res = _run(pkg, orc, 36.0, 99, "xy")
    rec, _, r_max = _fixture(pkg, 36.0)
    c3 = TC.create_cons3(x0, 100 / 180 * math.pi, np.full(N, 10.0))

    def poll_fn(Xs):
        bo, bi = np.inf, -1
        for k, v in enumerate(Xs):
            if c3(v):
                fv = orc.ref_objective(v, rec, r_max, 1e5)
                if fv < bo:
                    bo, bi = fv, k
        return bo, bi

    K = 2 * TS.polled_count(x0.size, "xy")
    assert K == 4 * N
    if mode == "sharded":
        g = _ThreadGather(world, lambda recs: d.reduce_best([r[0] for r in recs], [r[1] for r in recs]))
    else:
        g = _ThreadGather(world, lambda recs: recs)

    def body(r):
        shard = d.shard_range(K, r, world) if mode == "sharded" else None
        st = TS.PollStepper(x0, f0, poll_fn, seed=99, shard=shard, poll_vars="xy", **KW)
        loop = d.mads_loop if mode == "sharded" else d.mads_loop_speculative
        return loop(st, g.rank_view(r))

    for xs, st in _threads(world, body):
        assert np.array_equal(xs, want_x)
        assert st["f"] == want_f and st["iterations"] == res.status.iteration
        assert st["evaluations"] == 1 + K * res.status.iteration
