"""CPU: the cases of tests/weighted_mads_cases.py are what tests/test_gpu_mads_weighted.py needs them to
be: the lists (31 weights with exact sums; 10-90 % of the lattice overridden), every reference run no
trivial one and off the equal-weight run's iterate, the recipes of the issue's table at its counts, and
every case's plan on the fp64 credit rows of the build it is meant for."""
import numpy as np
import pytest

import shape_edges as se
import weighted_mads_cases as wc


def test_the_weighted_list(pkg):
    w = wc.weights(pkg)
    u = np.unique(w)
    assert w.size == 160 * 160 and u.size == 31 and u[0] == 0.25 and u[-1] == 7.75
    assert np.array_equal(u, 0.25 * np.arange(1, 32))
    assert float(np.add.accumulate(w)[-1]) == float(np.add.accumulate(w[::-1])[-1]) == w.sum() == 102449.25
    rec = wc.records(pkg)
    eq = wc.records(pkg, "equal")
    assert np.array_equal(rec[:, :2], eq[:, :2]) and np.array_equal(rec[:, 3], w) and np.all(eq[:, 3] == 25.0)


def test_the_regions_list(pkg):
    """Strictly between 10 % and 90 % of the entries overridden, inside both layouts' squares too."""
    rec = wc.records(pkg, "regions")
    hit = rec[:, 3] == wc.W_HI
    assert 0.1 < wc.override_fraction(pkg) == hit.mean() < 0.9
    assert set(np.unique(rec[:, 3])) == {25.0, wc.W_HI}
    for lo, span in ((320, 160), (380, 40)):
        box = (rec[:, 0] > lo - 36) & (rec[:, 0] < lo + span + 36) & (rec[:, 1] > lo - 36) & (rec[:, 1] < lo + span + 36)
        assert 0 < hit[box].sum() < box.sum()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_reference_runs(pkg, orc, name):
    ref = wc.conditions(pkg, orc, name)
    if name in wc.TABLE:
        assert (ref["succ"], ref["evals"]) == wc.TABLE[name]
    x0, _ = wc.start(pkg, name)
    N = wc.CASES[name]["N"]
    assert wc.candidates(name) >= se.kPollMinK
    if wc.CASES[name]["pv"] == "xy":
        assert ref["x"][2 * N:].tobytes() == x0[2 * N:].tobytes()


@pytest.mark.parametrize("name", ["band18", "band18m"])
def test_band_cases_reach_the_boundary(pkg, orc, name):
    """The start of each run has entries on its disks' boundaries (a candidate moves few disks, so nearly
    every candidate of the first polls keeps some); the cases on integer centres have none, at their start
    or their end (half-integer centres meet a few: (0, +-36) from a lattice entry)."""
    assert wc.boundary_entries(pkg, wc.start(pkg, name)[0]) >= 8
    for other in ("full", "xy18", "mesh"):
        assert wc.boundary_entries(pkg, wc.start(pkg, other)[0]) == 0
        assert wc.boundary_entries(pkg, wc.reference(pkg, orc, other)["x"]) == 0


@pytest.mark.parametrize("name", wc.REGION_CASES)
def test_reference_runs_on_the_regions_list(pkg, orc, name):
    ref = wc.conditions(pkg, orc, name, "regions")
    assert not np.array_equal(ref["x"], wc.reference(pkg, orc, name)["x"])


def test_the_barrier_run(pkg, orc):
    res = wc.prog_conditions(pkg, orc)[0]
    assert res.status.unsuccessful >= 1


def test_the_simulation_replay(pkg, orc):
    x0, want = wc.sim_replay(pkg, orc)
    assert [r["poll_vars"] for r in want] == ["xyr", "xy", "xy"]
    R = x0[2 * wc.SIM_N:]
    assert np.count_nonzero(R != R[-1]) == 2
    for r in want[1:]:   # (the held radii)
        assert r["x"][2 * wc.SIM_N:].tobytes() == r["input"][2 * wc.SIM_N:].tobytes()


@pytest.mark.parametrize("name", list(wc.CASES))
def test_plans(pkg, name):
    """counts == 0 on every plan; kMesh 0 / 1 / 2 by the mesh and the key mode; the fused chain where it
    is forced. The N = 513 block-edge polls: the full poll's K = 3078 is past the fused chain's limit
    (the five-launch chain runs whatever is forced), the xy poll's K = 2052 is not."""
    for keys in (False, True):
        wc.assert_route(pkg, name, "five", keys)
        wc.assert_route(pkg, name, "fused", keys)
    if name == "mesh":
        assert wc.assert_route(pkg, name, "fused", True, N=513, fused=0)["mesh"] == 2
    if name == "xy16":
        p = wc.assert_route(pkg, name, "fused", True, N=513)
        assert p["mesh"] == 2 and p["pair"] == 0 and p["gen_x"] == 0
        assert wc.assert_route(pkg, name, "fused", False, N=513)["mesh"] == 1
