"""CPU: keys in mesh units (MAC_OPT_MESH_KEYS; csrc/mesh_key.h). The header's pack, decode and
bit-for-bit check through the host-only mac_diag_mesh_key (the code the kernels inline) against numpy;
the Python mirror's polls against the decode of their draws; the option's ABI; and the route with the
key mode (mac_diag_route_keys: eval_plan and the chain word mac_mads_begin* derives)."""
import ctypes
import math
import os

import numpy as np
import pytest

from shape_edges import PLAN_FIELDS, SRC_GENERATED

KEY_ESC = 0x200 << 22
DEAD_WORD = KEY_ESC | 1
GS = (1.0, 2.0, 0.5, 0.125, 0.1, 0.005)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mesh_key(pkg, x, g, m, v=None):
    """mac_diag_mesh_key over n triples: (word[n], dec[n, 3], flags[n]); flags bit 0 packs, bit 1 exact."""
    L = pkg.load_library()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    L.mac_diag_mesh_key.argtypes = [ctypes.c_int64, dp, dp, ip, dp, ctypes.POINTER(ctypes.c_uint32), dp, ip]
    L.mac_diag_mesh_key.restype = ctypes.c_int32
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3)
    g = np.ascontiguousarray(np.broadcast_to(g, x.shape), dtype=np.float64)
    m = np.ascontiguousarray(np.broadcast_to(m, x.shape), dtype=np.int32)
    n = x.shape[0]
    word = np.zeros(n, dtype=np.uint32)
    dec = np.zeros((n, 3))
    flags = np.zeros(n, dtype=np.int32)
    vp = None
    if v is not None:
        v = np.ascontiguousarray(np.broadcast_to(v, x.shape), dtype=np.float64)
        vp = v.ctypes.data_as(dp)
    rc = L.mac_diag_mesh_key(n, x.ctypes.data_as(dp), g.ctypes.data_as(dp), m.ctypes.data_as(ip), vp,
                             word.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), dec.ctypes.data_as(dp),
                             flags.ctypes.data_as(ip))
    assert rc == 0
    return word, dec, flags


def _unpack(w):
    w = w.astype(np.int64)

    def sx(v, bits):
        return np.where(v >= 1 << (bits - 1), v - (1 << bits), v)
    return sx(w & 0x7FF, 11), sx((w >> 11) & 0x7FF, 11), sx((w >> 22) & 0x3FF, 10)


def _xs():
    t50 = math.tan(50 / 180 * math.pi)
    return np.array([0.0, 3.0, -17.0, 250.0, t50, 10 * t50, -7 * t50, 0.3, -0.0, 2.0 ** 53, 1e17])


@pytest.mark.parametrize("g", GS)
def test_round_trip_against_numpy(pkg, g):
    """decode(x, g, m) == x + g*m == the minus side x - g*|m| (m < 0), bit for bit, over m in
    [-1024, 1024]; the word holds the draws; it packs exactly when they fit the fields."""
    ms = np.arange(-1024, 1025, dtype=np.int32)
    for x in _xs():
        X = np.full((ms.size, 3), x)
        M = np.repeat(ms[:, None], 3, axis=1)
        plus = x + np.float64(g) * ms.astype(np.float64)
        # the candidate as the poll builds it: x + d or x - d with d = fl(g * L), L = |m|
        d = np.float64(g) * np.abs(ms).astype(np.float64)
        cand = np.where(ms >= 0, x + d, x - d)
        word, dec, flags = _mesh_key(pkg, X, g, M, v=np.repeat(cand[:, None], 3, axis=1))
        assert np.array_equal(_bits(dec[:, 0]), _bits(plus))
        assert np.array_equal(_bits(dec[:, 0]), _bits(cand))   # (x - d == x + (-d), -fl(g L) == fl(g (-L)))
        fits = np.abs(ms) <= 511   # (all three fields hold m: the r field is the narrowest)
        assert np.array_equal((flags & 1) != 0, fits)
        exact = _bits(dec) == _bits(np.repeat(cand[:, None], 3, axis=1))
        assert np.array_equal((flags & 2) != 0, exact.all(axis=1))
        ok = fits & exact.all(axis=1)
        assert np.all(word[~ok] == KEY_ESC)
        mx, my, mr = _unpack(word[ok])
        assert np.array_equal(mx, ms[ok]) and np.array_equal(my, ms[ok]) and np.array_equal(mr, ms[ok])
        assert not np.any(word[ok] == KEY_ESC) and not np.any(word[ok] == DEAD_WORD)
        assert exact.all(), (x, g)


def test_field_limits(pkg):
    """|m_x|, |m_y| <= 1023 and |m_r| <= 511 pack; one past does not, m_r = +-512 in particular (-512 is
    the escape pattern's r field); no packed word is the escape or the dead word."""
    x = np.array([[10.0, 20.0, 5.0]])
    for m, want in (((1023, -1023, 511), True), ((-1023, 1023, -511), True), ((1024, 0, 0), False),
                    ((0, -1024, 0), False), ((0, 0, 512), False), ((0, 0, -512), False), ((0, 0, 0), True),
                    ((1, 0, -511), True), ((0, 0, 1), True)):
        word, dec, flags = _mesh_key(pkg, x, (1.0, 0.5, 0.1), np.array([m], dtype=np.int32))
        assert bool(flags[0] & 1) == want, m
        assert (word[0] != KEY_ESC) == want, m
        assert word[0] != DEAD_WORD
        if want:
            assert tuple(int(a[0]) for a in _unpack(word)) == m
    # every r field over the whole range: never the escape's
    mr = np.arange(-511, 512, dtype=np.int32)
    M = np.stack([np.zeros_like(mr), np.ones_like(mr), mr], axis=1)
    word, _, flags = _mesh_key(pkg, np.tile(x, (mr.size, 1)), 0.125, M)
    assert np.all(flags == 3) and np.all((word >> 22) != 0x200)


def test_zero_draw_on_negative_zero_fails_the_check(pkg):
    """A held variable has m = 0 and its value is the incumbent's double as it is; on -0.0 the decode
    -0.0 + g * 0 is +0.0, another double: the check refuses the word."""
    x = np.array([[-0.0, 1.0, 2.0]])
    word, dec, flags = _mesh_key(pkg, x, 0.125, np.zeros((1, 3), dtype=np.int32), v=x)
    assert flags[0] == 1 and word[0] == KEY_ESC
    assert _bits(dec[0, 0]) == _bits(0.0) and _bits(dec[0, 0]) != _bits(-0.0)
    word, dec, flags = _mesh_key(pkg, np.abs(x), 0.125, np.zeros((1, 3), dtype=np.int32), v=np.abs(x))
    assert flags[0] == 3 and word[0] == 0
    # a polled variable's zero draw on -0.0: the plus candidate -0.0 + 0.0 is +0.0, the decode; the minus
    # candidate -0.0 - 0.0 is -0.0, which no draw decodes to (the one place -fl(g L) is not fl(g (-L)))
    plus = np.array([[np.float64(-0.0) + np.float64(0.0), 1.0, 2.0]])
    minus = np.array([[np.float64(-0.0) - np.float64(0.0), 1.0, 2.0]])
    assert _bits(plus[0, 0]) == _bits(0.0) and _bits(minus[0, 0]) == _bits(-0.0)
    assert _mesh_key(pkg, x, 0.125, np.zeros((1, 3), dtype=np.int32), v=plus)[2][0] == 3
    word, _, flags = _mesh_key(pkg, x, 0.125, np.zeros((1, 3), dtype=np.int32), v=minus)
    assert flags[0] == 1 and word[0] == KEY_ESC


def test_absorption_costs_a_position_only(pkg):
    """At |x| >= 2^53 two draws may decode to one double: both words are valid (each decodes to its
    candidate), they merely differ."""
    x = np.full((2, 3), 2.0 ** 53)
    M = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.int32)
    word, dec, flags = _mesh_key(pkg, x, 0.5, M)
    assert np.all(flags == 3) and word[0] != word[1] and _bits(dec[0, 0]) == _bits(dec[1, 0])


@pytest.mark.parametrize("poll_vars", ["xyr", "xy"])
@pytest.mark.parametrize("N", [3, 12])
def test_python_mirror_polls_are_the_decode_of_their_draws(pkg, N, poll_vars):
    """Every candidate of TDM_STATIC_opt's polls (poll_matrix over scaled_basis) equals the decode of
    its signed draw, ell = 0 .. 9; the words pack up to ell = 8 and the radius's diagonal +-512 at
    ell = 9 does not."""
    TS, wl = pkg.TDM_STATIC_opt, pkg.workloads
    n = 3 * N
    n_p = TS.polled_count(n, poll_vars)
    rng = wl.SplitMix64(41 + N)
    x = np.round(np.linspace(300.0, 420.0, n) * 8) / 8 + 0.3
    t50 = math.tan(50 / 180 * math.pi)
    x[2 * N:] = 10 * t50
    g = pkg._lib.mesh_granularity((0.5, 0.1), n)
    for ell in range(10):
        B = wl.ltmads_basis(n_p, ell, rng)
        X = TS.poll_matrix(x, TS.scaled_basis(B.astype(np.float64), g))
        Mfull = np.zeros((2 * n_p, n), dtype=np.int32)   # the signed draws; held variables 0
        Mfull[:n_p, :n_p] = B.T
        Mfull[n_p:, :n_p] = -B.T
        # disk i of candidate k: the triple of variables (i, N + i, 2N + i)
        idx = np.stack([np.arange(N), N + np.arange(N), 2 * N + np.arange(N)], axis=1)   # [N, 3]
        xs = np.tile(x[idx][None], (2 * n_p, 1, 1)).reshape(-1, 3)
        gs = np.tile(g[idx][None], (2 * n_p, 1, 1)).reshape(-1, 3)
        ms = Mfull[:, idx].reshape(-1, 3)
        vs = X[:, idx].reshape(-1, 3)
        word, dec, flags = _mesh_key(pkg, xs, gs, ms, v=vs)
        assert np.array_equal(_bits(dec), _bits(vs)), ell
        assert np.all((flags & 2) != 0)
        fits = (np.abs(ms[:, 0]) <= 1023) & (np.abs(ms[:, 1]) <= 1023) & (np.abs(ms[:, 2]) <= 511)
        assert np.array_equal((flags & 1) != 0, fits)
        assert np.all(word[~fits] == KEY_ESC) and not np.any(word[fits] == KEY_ESC)
        if ell <= 8:
            assert fits.all()
        elif poll_vars == "xyr":
            assert not fits.all() and np.all(np.abs(ms[~fits]).max(axis=1) == 512)
        # equal words of one disk are equal disks
        for i in range(N):
            wi, vi = word[i::N], vs[i::N]
            for w in np.unique(wi[wi != KEY_ESC]):
                rows = vi[wi == w]
                assert np.all(_bits(rows) == _bits(rows[0]))


def test_option_abi(pkg):
    """MAC_OPT_MESH_KEYS = 7: a null context is rejected whatever the value; the constants are the
    header's. (That 0 and 1 are accepted and 2 refused on a live context, before and after points are
    set, needs a device: tests/test_gpu_mesh_keys.py.)"""
    L = pkg.load_library()
    lib = pkg._lib
    assert (lib.MAC_OPT_MESH_KEYS, lib.MAC_KEYS_VALUE, lib.MAC_KEYS_MESH) == (7, 0, 1)
    for v in (0, 1, 2, -1):
        assert L.mac_set_option(None, lib.MAC_OPT_MESH_KEYS, v) == lib.MAC_E_INVAL
        assert "null" in L.mac_last_error().decode()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "maxcover.h")) as f:
        hdr = f.read().splitlines()
    for name, val in (("MAC_OPT_MESH_KEYS", 7), ("MAC_KEYS_VALUE", 0), ("MAC_KEYS_MESH", 1)):
        line = next(ln for ln in hdr if ln.startswith(f"#define {name} "))
        assert int(line.split()[2]) == val
    assert hasattr(pkg.Context, "set_mesh_keys")


def _route(pkg, N, K, keys, g, crowded=False, chain="auto", b=4, np_=0):
    L = pkg.load_library()
    lib = pkg._lib
    i64p = ctypes.POINTER(ctypes.c_int64)
    L.mac_diag_route_keys.argtypes = [i64p, ctypes.c_double, i64p, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_double), ctypes.c_int32, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int32)]
    L.mac_diag_route_keys.restype = ctypes.c_int32
    args = (lib.ALGOS["auto"], lib.CHAINS[chain], 256, 96 * 96, True, SRC_GENERATED, np_, 0, 0, False, 0, b,
            False, True, True, False, True, N, K, keys)
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    g = np.ascontiguousarray(g, dtype=np.float64)
    five = ctypes.c_int32(-1)
    rc = L.mac_diag_route_keys((ctypes.c_int64 * len(args))(*(int(a) for a in args)), 0.0, out, len(out),
                               g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if g.size else None, g.size,
                               int(crowded), ctypes.byref(five))
    return rc, dict(zip(PLAN_FIELDS, (int(v) for v in out))), five.value


def test_route(pkg):
    """(1, 0.1) on an uncrowded layout: AUTO plans the fused chain with mesh keys (the kMesh = 2 builds)
    and the five-launch chain with value keys (kMesh = 1); integer granularities and no mesh plan the
    same under both; a crowded layout goes to the five-launch chain under both; a bad mode is refused."""
    N, K = 12, 72
    g01 = np.r_[np.ones(2 * N), np.full(N, 0.1)]
    rc, p, five = _route(pkg, N, K, 1, g01)
    assert rc == 0 and five == 0 and p["fused_eligible"] == 1 and p["mesh"] == 2 and p["want_keys"] == 1
    rc, p, five = _route(pkg, N, K, 0, g01)
    assert rc == 0 and five == 1 and p["fused_eligible"] == 0 and p["mesh"] == 1
    rc, pf, _ = _route(pkg, N, K, 0, g01, chain="fused")   # (forced: value keys through the fused chain)
    assert rc == 0 and pf["fused_eligible"] == 1 and pf["mesh"] == 1
    for keys in (0, 1):
        rc, p, five = _route(pkg, N, K, keys, g01, crowded=True)
        assert rc == 0 and five == 1 and p["fused_eligible"] == 0 and p["mesh"] == 1 + keys
    # integer granularities: the same chain, each with its own builds
    g21 = np.r_[np.full(2 * N, 2.0), np.ones(N)]
    a, b = _route(pkg, N, K, 0, g21), _route(pkg, N, K, 1, g21)
    assert a[2] == b[2] == 0 and a[1]["fused_eligible"] == b[1]["fused_eligible"] == 1
    assert {k: v for k, v in a[1].items() if k != "mesh"} == {k: v for k, v in b[1].items() if k != "mesh"}
    # no mesh: identical plans
    a, b = _route(pkg, N, K, 0, np.zeros(0)), _route(pkg, N, K, 1, np.zeros(0))
    assert a == b and a[0] == 0 and a[1]["mesh"] == 0 and a[1]["fused_eligible"] == 1
    # an xy-only poll never steps by g_r: only the polled entries count
    rc, p, five = _route(pkg, N, 4 * N, 0, g01[:2 * N], np_=2 * N)
    assert rc == 0 and five == 0   # (K = 48 is below the poll chain: the chain word alone)
    assert _route(pkg, N, K, 2, g01)[0] == pkg._lib.MAC_E_INVAL
