"""CPU: the per-variable granularity (mac_mads_mesh, include/maxcover.h; DirectSearch's
SetGranularity, src/TDM_STATIC_opt.jl:131-137) on the host mirrors alone. Variable v steps by
fl(g[v] * L) with L the integer the stream draws on the unit mesh, and a candidate is x[v] + d or
x[v] - d: TDM_STATIC_opt.mads(granularity=) against that loop written out here one trial point and
one variable at a time; PollStepper follows mads; the auto rule compares with g_r / 2."""
import math

import numpy as np
import pytest

FOV = 100 / 180 * math.pi
TAN50 = math.tan(FOV / 2)
N = 3
KW = dict(N_iter=100, ell0=2, ell_max=5, seed=99)
_cache = {}


def _fixture(pkg):
    """test_gpu_poll_vars._recipe(3, 7, 320, 40): grid 160, radii 36.0, r_max = 30 tan 50 deg."""
    if "fx" not in _cache:
        wl = pkg.workloads
        x, y, w = wl.grid_points(160)
        rec = np.stack([x, y, w, w, np.zeros_like(x)], axis=1)
        rng = wl.SplitMix64(7)
        x0 = np.concatenate([np.round(320 + rng.uniform(N) * 40), np.round(320 + rng.uniform(N) * 40),
                             np.full(N, 36.0)])
        _cache["fx"] = rec, x0, np.full(N, 30.0 * TAN50)
    return _cache["fx"]


def _objective(pkg, orc):
    rec, x0, r_max = _fixture(pkg)
    c3 = pkg.TDM_Constraints.create_cons3(x0, FOV, np.full(N, 10.0))
    return (lambda v: orc.ref_objective(v, rec, r_max, 1e5)), [pkg.TDM_Constraints.cons1, c3]


def _written_out_loop(pkg, obj, cons, x0, g, n, N_iter, ell0, ell_max, seed):
    """The semantics, one product and one add per variable: (iterates, f, iterations, status)."""
    wl = pkg.workloads
    rng = wl.SplitMix64(seed)
    x = x0.copy()
    f = obj(x) if all(c(x) for c in cons) else math.inf
    ell, it, iterates = ell0, 0, []
    while it < N_iter and ell >= 0:
        it += 1
        B = wl.ltmads_basis(n, ell, rng)   # integers: B = L[rp][:, cp]
        bo, bx = math.inf, None
        for k in range(2 * n):
            kk = k if k < n else k - n
            v = x.copy()
            for q in range(n):
                d = float(g[q]) * float(B[q, kk])
                v[q] = x[q] + d if k < n else x[q] - d
            if all(c(v) for c in cons):
                fv = obj(v)
                if fv < bo:
                    bo, bx = fv, v
        if bx is not None and bo < f:
            x, f = bx, bo
            ell = min(ell + 1, ell_max)
        else:
            ell -= 1
        iterates.append(x.copy())
    return iterates, f, it, "MeshPrecisionLimit" if ell < 0 else "IterationLimit"


def _mads(pkg, orc, granularity, poll_vars="xyr", **kw):
    key = ("mads", repr(granularity), poll_vars, tuple(sorted(kw.items())))
    if key not in _cache:
        obj, cons = _objective(pkg, orc)
        _, x0, _ = _fixture(pkg)
        args = dict(KW, **kw)
        if granularity is not _NOKW:
            args["granularity"] = granularity
        _cache[key] = pkg.TDM_STATIC_opt.mads(x0, obj, cons, poll_vars=poll_vars, **args)
    return _cache[key]


_NOKW = object()


@pytest.mark.parametrize("gran", [(1.0, 0.1), (0.5, 0.125), (2.0, 1.0), (0.1, 0.1), 0.25, "vector"])
@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
def test_mads_against_the_written_out_loop(pkg, orc, gran, poll_vars):
    TS, lib = pkg.TDM_STATIC_opt, pkg._lib
    obj, cons = _objective(pkg, orc)
    _, x0, _ = _fixture(pkg)
    if gran == "vector":
        gran = np.array([1.0, 0.5, 0.25, 2.0, 1.0, 0.75, 0.1, 0.125, 0.3])
    g = lib.mesh_granularity(gran, x0.size)
    assert g.shape == (9,) and g.dtype == np.float64
    n = TS.polled_count(x0.size, poll_vars)
    iterates, f, it, status = _written_out_loop(pkg, obj, cons, x0, g, n, **KW)
    res = _mads(pkg, orc, gran if not isinstance(gran, np.ndarray) else tuple(gran), poll_vars)
    assert np.array_equal(res.x, iterates[-1]) and res.x_cost == f
    assert res.status.iteration == it and res.status.optimization_status == status
    assert f < obj(x0)
    if poll_vars == "xy":
        assert res.x[2 * N:].tobytes() == x0[2 * N:].tobytes()


def test_radius_granularity_removes_the_residual_penalty(pkg, orc):
    """The unit mesh keeps N * 0.2474 * 1e5 of penalty (r_max = 35.7526, integer radii); (1, 0.1) and
    (0.5, 0.125) get below it and stop at the mesh limit."""
    _, x0, r_max = _fixture(pkg)
    unit = _mads(pkg, orc, _NOKW)
    floor = N * (36.0 - r_max[0]) * 1e5
    assert np.array_equal(unit.x[2 * N:], np.full(N, 36.0))   # (integer radii: 36 is the nearest)
    # (a disk's covered cells have their centres inside it: their area is below (2 r + pitch)^2)
    assert unit.x_cost > floor - N * (2 * 36.0 + pkg.workloads.PITCH) ** 2
    for gran in ((1.0, 0.1), (0.5, 0.125)):
        res = _mads(pkg, orc, gran)
        assert res.x_cost < floor / 2 and res.x_cost < unit.x_cost
        assert res.status.optimization_status == "MeshPrecisionLimit" and res.status.iteration < 100
        assert np.all(res.x[2 * N:] != np.round(res.x[2 * N:]))
    r = _mads(pkg, orc, (0.5, 0.125)).x
    assert np.array_equal(r * 8, np.round(r * 8))   # every value on the 0.125 (and 0.5) mesh


@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
def test_unit_granularity_is_the_call_without_the_keyword(pkg, orc, poll_vars):
    base = _mads(pkg, orc, _NOKW, poll_vars)
    for gran in (None, 1.0, tuple(np.ones(3 * N))):
        res = _mads(pkg, orc, gran, poll_vars)
        assert res.x.tobytes() == base.x.tobytes() and res.x_cost == base.x_cost
        assert res.status.iteration == base.status.iteration
        assert res.status.function_evaluations == base.status.function_evaluations
        assert res.status.successes == base.status.successes
    # ... and every poll matrix: scaling by ones is the identity on the basis's doubles
    TS, wl = pkg.TDM_STATIC_opt, pkg.workloads
    B = wl.ltmads_basis(9, 4, wl.SplitMix64(3)).astype(np.float64)
    assert TS.scaled_basis(B, None) is B
    assert TS.scaled_basis(B, np.ones(9)).tobytes() == B.tobytes()


def test_scaled_basis_is_one_product_per_row(pkg):
    TS, wl = pkg.TDM_STATIC_opt, pkg.workloads
    g = np.array([0.1, 0.3, 1.0, 2.0, 0.125, 0.7])
    B = wl.ltmads_basis(6, 3, wl.SplitMix64(11)).astype(np.float64)
    S = TS.scaled_basis(B, g)
    for v in range(6):
        for k in range(6):
            assert S[v, k] == g[v] * B[v, k]
    # an xy-only poll's basis (n_p = 4 of 6 variables) takes the first n_p entries
    B4 = wl.ltmads_basis(4, 2, wl.SplitMix64(11)).astype(np.float64)
    assert np.array_equal(TS.scaled_basis(B4, g), g[:4, None] * B4)


@pytest.mark.parametrize("gran", [(1.0, 0.1), (0.5, 0.125)])
def test_poll_stepper_follows_mads(pkg, orc, gran):
    """poll / update, and poll_ahead / advance with ahead <= 2, end on mads's iterate."""
    TS = pkg.TDM_STATIC_opt
    obj, cons = _objective(pkg, orc)
    _, x0, _ = _fixture(pkg)
    want = _mads(pkg, orc, gran)

    def poll_fn(Xs):
        bo, bi = math.inf, -1
        for k, v in enumerate(Xs):
            if all(c(v) for c in cons):
                fv = obj(v)
                if fv < bo:
                    bo, bi = fv, k
        return bo, bi

    st = TS.PollStepper(x0, obj(x0), poll_fn, granularity=gran, **KW)
    while True:
        done, bo, bi = st.poll()
        if done:
            break
        st.update(bo, bi)
    xs, s = st.result()
    assert np.array_equal(xs, want.x) and s["f"] == want.x_cost
    assert s["iterations"] == want.status.iteration and s["status"] == 0

    sp = TS.PollStepper(x0, obj(x0), poll_fn, granularity=gran, **KW)
    finished = False
    while not finished:
        res = [sp.poll_ahead(j) for j in range(3)]
        for done, bo, bi, _ in res:
            if done:
                finished = True
                break
            if sp.advance(bo, bi):
                break
    xs, s = sp.result()
    assert np.array_equal(xs, want.x) and s["f"] == want.x_cost
    assert s["iterations"] == want.status.iteration and s["status"] == 0


def test_auto_rule_at_half_the_radius_granularity(pkg):
    """"xy" iff every |R_i - r_max_i| <= g_r / 2: g_r = 0.25, at 0.125 exactly and at both
    neighbouring doubles, either side of r_max; the two-argument call keeps 0.5."""
    auto = pkg.FullSimulation.auto_poll_vars
    rm = np.array([36.0, 36.0, 20.0])   # (exact doubles: the differences below are exact, Sterbenz)
    h = 0.125
    assert auto(rm + h, rm, 0.25) == "xy" and auto(rm - h, rm, 0.25) == "xy"
    assert auto(np.nextafter(rm + h, rm), rm, 0.25) == "xy" and auto(np.nextafter(rm - h, rm), rm, 0.25) == "xy"
    for i in range(3):
        for sg in (1.0, -1.0):
            R = rm.copy()
            R[i] = np.nextafter(rm[i] + sg * h, sg * np.inf)
            assert abs(R[i] - rm[i]) > h
            assert auto(R, rm, 0.25) == "xyr"
            assert auto(R, rm) == "xy"   # (0.5 without g_r)
    # per-UAV granularities
    g3 = np.array([1.0, 0.25, 0.125])   # (halves exact in binary)
    assert auto(rm + g3 / 2, rm, g3) == "xy" and auto(rm - g3 / 2, rm, g3) == "xy"
    for i in range(3):
        R = rm + g3 / 2
        R[i] = np.nextafter(R[i], np.inf)
        assert auto(R, rm, g3) == "xyr"
    assert auto(rm + 0.5, rm) == "xy" and auto(rm + 0.5, rm, 1.0) == "xy"
    assert auto(np.nextafter(rm + 0.5, np.inf), rm) == "xyr"


def test_granularity_forms(pkg):
    mg = pkg._lib.mesh_granularity
    assert mg(None, 9) is None
    assert np.array_equal(mg(0.5, 9), np.full(9, 0.5))
    assert np.array_equal(mg((0.5, 0.125), 9), [0.5] * 6 + [0.125] * 3)
    v = np.arange(1.0, 10.0)
    assert np.array_equal(mg(v, 9), v) and np.array_equal(mg(list(v), 9), v)
    assert np.array_equal(mg(np.array([2.0, 3.0, 4.0]), 3), [2.0, 3.0, 4.0])   # N = 1: a vector, not a pair
    assert np.array_equal(mg((2.0, 3.0), 3), [2.0, 2.0, 3.0])


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, math.inf, (1.0, 0.0), (math.nan, 1.0), (1.0, 2.0, 3.0),
                                 "vector_with_zero", "wrong_length", "matrix", "text"])
def test_value_errors_name_granularity(pkg, bad):
    TS, FS, lib = pkg.TDM_STATIC_opt, pkg.FullSimulation, pkg._lib
    x0 = np.zeros(9)
    if bad == "vector_with_zero":
        bad = np.array([1.0] * 8 + [0.0])
    elif bad == "wrong_length":
        bad = np.ones(8)
    elif bad == "matrix":
        bad = np.ones((3, 3))
    with pytest.raises(ValueError, match="granularity"):
        lib.mesh_granularity(bad, 9)
    with pytest.raises(ValueError, match="granularity"):
        TS.mads(x0, lambda v: 0.0, granularity=bad)
    with pytest.raises(ValueError, match="granularity"):
        TS.PollStepper(x0, 0.0, lambda Xs: (math.inf, -1), granularity=bad)
    # before the context or the library is touched (a context of None would fail otherwise)
    with pytest.raises(ValueError, match="granularity"):
        FS.Simulation(None, x0, initial_points=np.zeros((0, 5)), granularity=bad)
    with pytest.raises(ValueError, match="granularity"):
        lib.Context.mads_run(None, x0, np.ones(3), granularity=bad)
    with pytest.raises(ValueError, match="granularity"):
        lib.Context.mads_stepper(None, x0, np.ones(3), granularity=bad)
