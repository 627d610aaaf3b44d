"""GPU: the fused chain's matrix-source prep (k_prep.h prep_x_kernel<false>) at the edges of its
slot layout and of its displacement bound. Workgroup cw takes candidates 6cw .. 6cw + 5 and, in the
first K mod 6 workgroups, candidate xbase + cw (xbase = 6 (K // 6)) in a seventh slot; the other
workgroups skip that slot's arithmetic. The bound ({max |x - x0|, max |y - y0|, max r - r0, max
r0 - r} over the live candidates, k_fiw.h sup_box) comes from the packed keys' integer offsets,
and in fp64 for the candidates whose keys escape.

Every case: a 64 x 64 lattice, a candidate matrix on the device, a fresh context with the fused
chain forced (its three launches asserted), every objective and the argmin == the oracle's
(-PointerList.area_batch + violation_batch * penalty, +inf where cons3_batch fails) and == the
five-launch chain's. Reference: src/AreaCoverageCalculation.jl:63-78, src/TDM_STATIC_opt.jl:82-100,
src/TDM_Constraints.jl:54-75."""
import math

import numpy as np
import pytest
import torch

from test_gpu_parity import recs

pytestmark = pytest.mark.gpu
TAN50 = math.tan(100 / 180 * math.pi / 2)
G = 64          # lattice cells a side (5 m pitch: 320 m)
PEN = 1e5
R0 = 20.0       # candidate 0's radii


@pytest.fixture(scope="module")
def lattice(pkg, orc):
    """(x, y, w, the oracle's point list): built once, read only."""
    x, y, w = pkg.workloads.grid_points(G)
    return x, y, w, orc.PointerList(recs(x, y, w))


def make_poll(pkg, N, K, seed, sign=None):
    """K x 3N: candidate 0 with integer centres inside the lattice and r = R0, every other
    candidate within +-4 of it in every variable (integers: every key packs). sign = (variable
    index, +1 | -1): that variable's offsets lie on one side, in [0, 4] or [-4, 0], so that a
    mover of the full field width in candidate 0 itself leaves the others inside the field."""
    rng = pkg.workloads.SplitMix64(seed)
    base = np.concatenate([rng.integers(40, 280, 2 * N).astype(np.float64), np.full(N, R0)])
    off = rng.integers(-4, 4, K * 3 * N).reshape(K, 3 * N).astype(np.float64)
    off[0] = 0.0
    if sign is not None:
        v, s = sign
        off[:, v] = s * np.abs(off[:, v])
    return base[None, :] + off


def want_objs(orc, lattice, C, rmax, prev, dlim):
    N = C.shape[1] // 3
    want = -lattice[3].area_batch(C)
    if rmax is not None:
        want = want + orc.violation_batch(C, rmax) * PEN
    if prev is not None:
        want = np.where(orc.cons3_batch(prev, C, dlim, TAN50), want, np.inf)
    assert want.shape == (C.shape[0],) and N > 0
    return want


def dev_poll(c, dev, C, rmax, prev, dlim):
    """One device poll on context c: (objectives, (best, index), {kernel: launches})."""
    K, n3 = C.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    dC, dR, dP, dL = t(C), t(rmax), t(prev), t(dlim)
    dB = torch.empty(2, dtype=torch.float64, device=dev)
    dO = torch.empty(K, dtype=torch.float64, device=dev)
    c.profile(True)
    c.profile_read(reset=True)
    c.poll_best_dev(dC, n3, K, dR, dB, PEN, d_prev=dP, d_dlim=dL, tan_half_fov=TAN50, d_obj=dO)
    torch.cuda.synchronize()
    best = c.best_fetch(dB)
    kern = {k: n for k, (ms, n) in c.profile_kernels().items() if n}
    c.profile_read(reset=True)
    return dO.cpu().numpy(), best, kern


def assert_fused(kern):
    # (role 0 is the chain's prep launch: prep_x_kernel on this route)
    assert kern.get("prep_kernel", 0) > 0 and kern.get("fiw_kernel", 0) > 0 and kern.get("fin2_kernel", 0) > 0, kern


def check(pkg, orc, lattice, polls, rmax="default", prev=None, dlim=None):
    """The polls (a list of candidate matrices, in order on one fresh context) through the forced
    fused chain, then through the five-launch chain, each against the oracle."""
    x, y, w, _ = lattice
    dev = torch.device("cuda", 0)
    with pkg.Context(0) as c:
        c.set_points(x, y, w)
        for chain in ("fused", "five"):
            c.set_chain(chain)
            for C in polls:
                N = C.shape[1] // 3
                rm = np.full(N, 25.0) if isinstance(rmax, str) else rmax
                pv = prev(C) if callable(prev) else prev
                dl = None if pv is None else np.full(N, 10.0) if dlim is None else dlim
                want = want_objs(orc, lattice, C, rm, pv, dl)
                assert np.isfinite(want).any()
                got, (bo, bi), kern = dev_poll(c, dev, C, rm, pv, dl)
                if chain == "fused":
                    assert_fused(kern)
                else:
                    assert "fiw_kernel" not in kern, kern
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (chain, C.shape, bad[:6], got[bad[:6]], want[bad[:6]])
                k = int(np.argmin(want))
                assert bi == k and bo == want[k], (chain, bi, k)


def slot_candidate(K, where):
    """Slot 0 of workgroup 0, slot 5 of the last workgroup, the first remainder slot (xbase)."""
    xbase = 6 * (K // 6)
    return {"first": 0, "last": xbase - 1, "rem": xbase}[where]


# ---------------------------------------------------------------- remainders

@pytest.mark.parametrize("N,K", [(5, 66), (5, 67), (5, 71), (5, 72), (5, 73), (512, 67)])
def test_remainders(pkg, orc, lattice, N, K):
    """K mod 6 = 0, 1, 5, 0, 1: the last workgroup with a seventh slot beside the first without
    one. With cons3 (prev = candidate 0, d_lim = 10): failures in the last candidate (a remainder
    slot when K mod 6 != 0), in workgroup 0 and in the last workgroup's slot 5, so a failure bit of
    slot 6 must not leak into a workgroup that has none."""
    C = make_poll(pkg, N, K, 100 + K + N)
    for k, i in ((K - 1, 0), (3, N - 1), (6 * (K // 6) - 1, N // 2)):
        C[k, N + i] += 15.0
    check(pkg, orc, lattice, [C])
    check(pkg, orc, lattice, [C], prev=lambda M: M[0].copy())


# ---------------------------------------------------------------- the far candidate

# (variable of UAV 0: 0 x, 1 y, 2 r; the move; candidate 0's value of it). Candidate 0's disk lies off
# the lattice for the centre moves and the mover lands in its middle, so a bound that missed the
# mover would leave the mover's entries out of UAV 0's box; r + 511 grows the disk over the whole
# lattice, r - 511 shrinks a disk that covers it to 20 m (the bound's fourth component).
MOVES = {"x+1023": (0, 1023.0, 160.0 - 1023.0), "y-1023": (1, -1023.0, 160.0 + 1023.0),
         "r+511": (2, 511.0, R0), "r-511": (2, -511.0, R0 + 511.0)}


def far_poll(pkg, K, move, where, amount=None, seed=7):
    N = 5
    q, d, v0 = MOVES[move]
    d = d if amount is None else amount
    var = q * N   # (UAV 0's)
    C = make_poll(pkg, N, K, seed, sign=(var, 1.0 if d > 0 else -1.0))
    C[:, var] += v0 - C[0, var]
    if q == 2:
        C[:, 0] += 160.0 - C[0, 0]
        C[:, N] += 160.0 - C[0, N]
    k = slot_candidate(K, where)
    C[k, var] = v0 + d
    return C, k


@pytest.mark.parametrize("where", ["first", "last", "rem"])
@pytest.mark.parametrize("move", list(MOVES))
def test_bound_covers_the_far_candidate(pkg, orc, lattice, move, where):
    """Exactly one candidate moves UAV 0 by the full width of a key field (+1023 in x, -1023 in y,
    +-511 in r), all the others within +-4: the mover's area, and every other candidate's, equals
    the oracle's. (The mover in candidate 0 is the keys' base: every other candidate then lies the
    field's width away, on the side that still packs.)"""
    C, k = far_poll(pkg, 67, move, where)
    q, d, _ = MOVES[move]
    far = np.abs(C[:, q * 5] - C[0, q * 5])
    others = np.delete(far, k)[1 if k else 0:]
    assert far.max() == abs(d) and ((others >= abs(d) - 4).all() if k == 0 else (others <= 4).all())
    check(pkg, orc, lattice, [C])


# ---------------------------------------------------------------- escapes beside packed keys

@pytest.mark.parametrize("where", ["first", "last", "rem"])
@pytest.mark.parametrize("amount", [1024.0, 1000.5])
def test_escaped_far_candidate(pkg, orc, lattice, amount, where):
    """The mover one past the x field (+1024: x alone escapes) and at a non-integer offset
    (+1000.5): its share of the bound comes from the fp64 path, the others' from their integers."""
    C, _ = far_poll(pkg, 67, "x+1023", where, amount=amount)
    check(pkg, orc, lattice, [C])


def test_two_escapes_in_one_thread(pkg, orc, lattice):
    """Two escaped candidates of UAV 0 in one workgroup (slots 0 and 2 of workgroup 1: +1024 in x,
    +0.5 in y and 300.5 in r) beside four packed ones, and one in the remainder slot."""
    C, _ = far_poll(pkg, 67, "x+1023", "last", amount=3.0)
    C[6, 0] = C[0, 0] + 1024.0
    C[8, 5] += 0.5
    C[8, 10] += 300.5
    C[66, 0] = C[0, 0] + 1030.0
    check(pkg, orc, lattice, [C])


# ---------------------------------------------------------------- slots that are not live

@pytest.mark.parametrize("where", ["last", "rem"])
@pytest.mark.parametrize("r", [0.0, -3.0])
def test_far_candidate_without_a_disk(pkg, orc, lattice, r, where):
    """The candidate with the largest offset has r = 0 or r < 0 for that UAV: it covers nothing and
    is left out of the bound; a second, live mover (+1000, inside the lattice) sets it."""
    C, k = far_poll(pkg, 67, "x+1023", where)
    C[k, 10] = r
    C[7, 0] = C[0, 0] + 1000.0
    check(pkg, orc, lattice, [C])


@pytest.mark.parametrize("where", ["first", "last", "rem"])
def test_far_candidate_beside_nan_and_inf_centres(pkg, orc, lattice, where):
    """A NaN and a +inf centre (not live: no disk) in the mover's workgroup and in another one."""
    C, k = far_poll(pkg, 67, "y-1023", where)
    # (the mover's workgroup: candidates 0 .. 5 and 66, or 60 .. 65; candidate 0 stays as it is)
    a, b = (k - 1, k - 2) if where == "last" else (1, 2)
    C[a, 0] = np.nan
    C[b, 5 + 1] = np.inf
    C[30, 2] = np.nan
    C[31, 0] = np.inf
    check(pkg, orc, lattice, [C])


@pytest.mark.parametrize("where", ["last", "rem"])
def test_cons3_failure_carries_the_largest_offset(pkg, orc, lattice, where):
    """prev = candidate 0, d_lim = 10: the far candidate fails cons3, is left out of the bound and
    reads +inf; a workgroup whose six candidates all fail (workgroup 2: candidates 12 .. 17)."""
    C, k = far_poll(pkg, 67, "x+1023", where)
    C[12:18, 5 + 1] += 15.0
    prev = C[0].copy()
    feas = orc.cons3_batch(prev, C, np.full(5, 10.0), TAN50)
    assert not feas[k] and not feas[12:18].any() and int(feas.sum()) == 67 - 7
    check(pkg, orc, lattice, [C], prev=prev)


# ---------------------------------------------------------------- no penalty inputs

def test_without_r_max(pkg, orc, lattice):
    """No r_max (the penalty term is 0), cons3 on: a failure in the remainder slot."""
    C = make_poll(pkg, 5, 67, 41)
    C[66, 5] += 15.0
    C[20, 1] -= 15.0
    check(pkg, orc, lattice, [C], rmax=None, prev=lambda M: M[0].copy())


def test_without_prev(pkg, orc, lattice):
    """No prev (no cons3): nothing is dead, whatever candidate moves 15 m."""
    C = make_poll(pkg, 5, 67, 42)
    C[66, 5] += 15.0
    C[20, 1] -= 15.0
    check(pkg, orc, lattice, [C])


# ---------------------------------------------------------------- successive polls

def test_successive_polls_with_and_without_a_seventh_slot(pkg, orc, lattice):
    """K = 73 (workgroup 0 has a seventh slot, whose candidate fails cons3), then K = 66 (no
    workgroup has one) on the same context: nothing of the first poll's slot 6 survives."""
    A = make_poll(pkg, 5, 73, 51)
    A[72, 5] += 15.0
    B = make_poll(pkg, 5, 66, 52)
    check(pkg, orc, lattice, [A, B], prev=lambda M: M[0].copy())
    check(pkg, orc, lattice, [A, B])
