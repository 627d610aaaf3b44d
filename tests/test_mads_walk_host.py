"""CPU: the native MADS driver's host arithmetic (csrc/mads_walk.h: the stream's states, the
permutations of every iteration and of the polls drawn ahead, the point of a chosen candidate, the
acceptance rule) against TDM_STATIC_opt.PollStepper. The stepper runs here on plain numpy with a Python
objective and records, per iteration, the permutations (workloads.ltmads_basis_parts on a copy of its
stream), the poll's outcome and the state it leaves; tests/host/mads_walk_check.cpp, built with the host
compiler (no FMA contraction, as the library's build), replays the outcomes through mads_walk.h and
compares everything byte for byte. The same program runs a second time under the address and
undefined-behaviour sanitizers.

The objective is max(|x - t|^2, floor): t lies off the mesh, 13.37 from x0 in every polled variable,
so polls succeed at first (ell0 = 1 < ell_max = 2: a refinement, then successes clamped at ell_max);
under the floor nothing improves strictly, and the run ends by ell < 0 after failures at every ell. Every
case asserts that its run has all of these, so none passes on an empty or one-sided record."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "maximumareacoverageoptimization.jl_amd", "csrc")
ELL0, ELL_MAX, N_ITER, SEED = 1, 2, 120, 20250216
AHEAD = (0, 1, 3)
# the floor as a share of f(x0), per n_p: low enough for a success at ell_max, reached within N_ITER
FLOOR = {2: 0.02, 3: 0.02, 4: 0.02, 6: 0.02, 22: 0.6, 33: 0.6, 342: 0.985, 513: 0.985}


@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    """The replay program, plain and under the sanitizers (stand-alone programs: nothing preloaded)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the package's own build needs one)")
    d = tmp_path_factory.mktemp("mads_walk")
    src = os.path.join(ROOT, "tests", "host", "mads_walk_check.cpp")
    base = [cxx, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC]
    plain, san = str(d / "mads_walk_check"), str(d / "mads_walk_check_san")
    subprocess.run(base + ["-O1", "-o", plain, src], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", san, src], check=True)
    return plain, san


def _perms_ahead(pkg, st, ahead):
    """(rp, cp) of the iteration `ahead` after the stepper's current one: ltmads_basis_parts's own draws
    on a copy of the stream, one call per iteration (ell does not move the permutations)."""
    rng = pkg.workloads.SplitMix64()
    rng.state = st.rng.state
    for _ in range(ahead + 1):
        _, rp, cp = pkg.workloads.ltmads_basis_parts(st.n, 0, rng)
    return rp, cp


def _record(pkg, path, N, poll_vars, granularity, speculate):
    """Runs the stepper, writes the record (mads_walk_check.cpp's format), returns the outcomes as
    [(ell of the poll, moved)]."""
    TS = pkg.TDM_STATIC_opt
    i = np.arange(N, dtype=np.float64)
    x0 = np.concatenate([100.0 + 7.3 * i, 50.0 + 3.7 * i, 30.1 + 0.3 * i])
    n = x0.size
    n_p = TS.polled_count(n, poll_vars)
    t = x0.copy()
    t[:n_p] += 13.37
    f0 = float(np.sum((x0 - t) ** 2))
    floor = FLOOR[n_p] * f0

    def poll_fn(X):
        q = np.maximum(np.sum((X - t[None, :]) ** 2, axis=1), floor)
        k = int(np.argmin(q))
        return float(q[k]), k

    st = TS.PollStepper(x0, f0, poll_fn, N_iter=N_ITER, ell0=ELL0, ell_max=ELL_MAX, seed=SEED,
                        poll_vars=poll_vars, granularity=granularity)
    g = st.g
    out = [struct.pack("<5qQ", n, n_p, 0 if g is None else 1, ELL0, ELL_MAX, SEED)]
    recs, outcomes = [], []
    while True:
        probes = [(a,) + _perms_ahead(pkg, st, a) for a in (AHEAD if speculate else (0,))]
        ell = st.ell
        if speculate:
            polls = [st.poll_ahead(a) for a in AHEAD]
            done, bo, bi = polls[0][:3]
            if done:
                break
            moved = st.advance(bo, bi)
        else:
            done, bo, bi = st.poll()
            if done:
                break
            f_was = st.f
            st.update(bo, bi)
            moved = bi >= 0 and bo < f_was
        outcomes.append((ell, bool(moved)))
        r = [struct.pack("<q", len(probes))]
        for a, rp, cp in probes:
            r += [struct.pack("<q", a), rp.astype("<i4").tobytes(), cp.astype("<i4").tobytes()]
        r += [struct.pack("<dq", bo, bi), st.x.astype("<f8").tobytes(),
              struct.pack("<dqQ", st.f, st.ell, int(st.rng.state))]
        recs.append(b"".join(r))
    out += [struct.pack("<q", len(recs)), x0.astype("<f8").tobytes(), struct.pack("<d", f0)]
    if g is not None:
        out.append(np.asarray(g, dtype="<f8").tobytes())
    out += recs
    out.append(struct.pack("<2q", sum(m for _, m in outcomes), st.it))
    with open(path, "wb") as fh:
        fh.write(b"".join(out))
    assert st.it == len(outcomes)
    return outcomes, st


@pytest.mark.parametrize("speculate", [False, True], ids=["update", "advance"])
@pytest.mark.parametrize("granularity", [None, (1.0, 0.125)], ids=["nomesh", "mesh"])
@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
@pytest.mark.parametrize("N", [1, 2, 11, 171])
def test_walk_replays_the_stepper(pkg, checkers, tmp_path, N, poll_vars, granularity, speculate):
    path = str(tmp_path / "run.bin")
    outcomes, st = _record(pkg, path, N, poll_vars, granularity, speculate)
    seq = "".join("S" if m else "f" for _, m in outcomes)
    print(f"N={N} {poll_vars} n_p={st.n} iterations {st.it}: {seq}")
    # the run is no trivial one: a success, a failure, a success on a poll at ell_max (the clamp), and
    # its end by ell < 0 (not by the iteration limit)
    assert any(m for _, m in outcomes) and any(not m for _, m in outcomes)
    assert any(m and ell < ELL_MAX for ell, m in outcomes)
    assert any(m and ell == ELL_MAX for ell, m in outcomes)
    assert st.ell < 0 and st.it < N_ITER
    for exe in checkers:
        r = subprocess.run([exe, path], capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert f"records {st.it} " in r.stdout and r.stdout.rstrip().endswith(": ok")
