"""ctypes binding of libmaxcover.so (include/maxcover.h).

This is the Python stand-in for the Julia ``ccall`` shim (julia/MaxCoverAMD.jl): same entry
points, same array layouts, same error behaviour. There is no CPU fallback: if the shared
library is missing or cannot be loaded, every entry point raises ``MaxCoverError``.
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MAXCOVER_LIB") or os.path.join(_HERE, "libmaxcover.so")

MAC_OK = 0
MAC_E_INVAL = 1
MAC_E_SIZE = 2
MAC_E_NOPOINTS = 3
MAC_E_HIP = 4
MAC_E_NOMEM = 5
MAC_E_LOSSY = 6
MAC_E_NODEVICE = 7

MAC_OPT_ALGO = 1
MAC_OPT_STORAGE = 2
MAC_OPT_TILE_POINTS = 3
MAC_OPT_PROFILE = 4
MAC_OPT_SHARED = 5
MAC_OPT_CHAIN = 6
MAC_OPT_MESH_KEYS = 7
MAC_OPT_VERDICTS = 8
MAC_KEYS_VALUE = 0
MAC_KEYS_MESH = 1
SHARED_MODES = {"auto": 0, "fp64": 1, "bits": 2}
CHAINS = {"auto": 0, "five": 1, "fused": 2}
MAC_ALGO_AUTO = 0
MAC_ALGO_SCAN = 1
MAC_ALGO_TILED = 2
MAC_ALGO_POLL = 3
MAC_STORE_F64 = 0
MAC_STORE_F32 = 1

# mac_profile_kernels launch roles (include/maxcover.h MAC_PROF_ROLES). Role 5 is one stamp slot
# for the crowded-poll shared-entry pass: the union pass (shared_or_kernel) on equal weights — every
# reference data set — else the bit-word kernel (shared_bits_kernel)
PROF_ROLES = ("prep_kernel",  # (role 0: the prep launch, prep_kernel or prep_x_kernel)
              "disk_index_kernel", "walk_setup_kernel", "coverage_tiled_poll_kernel",
              "coverage_poll_kernel", "shared_or_kernel", "finalize_kernel", "fiw_kernel",
              "fin2_kernel", "cons_mask_gen_kernel", "prog_h_kernel", "prog_select_kernel")

# mac_diag_poll_report: the poll walk's counters in their order (csrc/k_common.h kDc*)
POLL_COUNTERS = ("bits", "poll_jobs", "other", "bits_jobs", "or_jobs0", "or_jobs1", "or_jobs2",
                 "or_jobs3", "or_bad")

ALGOS = {"auto": MAC_ALGO_AUTO, "scan": MAC_ALGO_SCAN, "tiled": MAC_ALGO_TILED,
         "poll": MAC_ALGO_POLL}

# Every symbol include/maxcover.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "mac_last_error", "mac_version", "mac_device_count", "mac_ctx_create", "mac_ctx_destroy",
    "mac_set_option", "mac_set_points_f64", "mac_set_points_records_f64",
    "mac_set_points_dev_f64", "mac_num_points", "mac_get_points_f64",
    "mac_remove_covered_f64", "mac_covered_flags_f64", "mac_area_f64", "mac_area_batch_f64",
    "mac_objective_batch_f64", "mac_poll_best_f64", "mac_area_batch_dev_f64",
    "mac_poll_best_dev_f64", "mac_best_fetch", "mac_poll_arm_dev_f64", "mac_poll_fire",
    "mac_cover_threshold", "mac_profile_read",
    "mac_profile_split", "mac_profile_kernels",
    "mac_append_points_f64", "mac_append_points_dev_f64", "mac_mads_run",
    "mac_fire_last_error", "mac_fire_thresholds", "mac_fire_create", "mac_fire_destroy",
    "mac_fire_initial_points", "mac_fire_step", "mac_fire_last_points", "mac_fire_get_grid",
    "mac_fire_set_grid",
    "mac_set_points_f32", "mac_set_points_dev_f32", "mac_area_f32", "mac_area_batch_f32",
    "mac_poll_best_f32", "mac_poll_best_dev_f32",
    "mac_mads_begin", "mac_mads_poll", "mac_mads_update", "mac_mads_result", "mac_mads_destroy",
    "mac_mads_poll_ahead", "mac_mads_advance",
    "mac_mads_best_buffer", "mac_best_reduce_dev", "mac_poll_basis_f64",
    "mac_comm_unique_id", "mac_comm_init", "mac_poll_exchange", "mac_exchange_records",
    "mac_area_by_disk_f64", "mac_area_by_disk_batch_f64", "mac_area_by_disk_dev_f64",
    "mac_cons_mask_f64", "mac_cons_mask_dev_f64", "mac_poll_best_cons_f64",
    "mac_poll_best_cons_dev_f64", "mac_mads_run_cons", "mac_mads_begin_cons",
    "mac_set_regions", "mac_regions_ingested", "mac_region_stats_f64",
    "mac_mads_run_opts", "mac_mads_begin_opts",
    "mac_cons_mask_motion_f64", "mac_poll_best_motion_f64", "mac_motion_thresholds",
    "mac_mads_run_motion", "mac_mads_begin_motion",
    "mac_mads_run_mesh", "mac_mads_begin_mesh", "mac_profile_fused",
    "mac_prog_h_f64", "mac_mads_run_prog", "mac_diag_poll_report",
    "mac_mads_begin_prog", "mac_mads_poll_prog", "mac_prog_merge", "mac_mads_advance_prog",
    "mac_mads_result_prog",
    "mac_cons_explain_f64", "mac_verdict_read",
)

MAC_REGIONS_MAX = 64


def high_interest_mask(x, y, boxes) -> np.ndarray:
    """The reference's high-interest test (src/CellFunctions.jl:42, :68; src/FullSimulation.jl:542)
    for arrays of points: ``x < x_UB && x > x_LB && y < y_UB && y > y_LB`` (all strict) for any
    box of ``boxes = (x_LB, x_UB, y_LB, y_UB)`` (equal-length sequences). The single host
    restatement of the test mac_set_regions applies on the device."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x_LB, x_UB, y_LB, y_UB = boxes
    m = np.zeros(np.broadcast(x, y).shape, dtype=bool)
    for xl, xu, yl, yu in zip(x_LB, x_UB, y_LB, y_UB):
        m |= (x < xu) & (x > xl) & (y < yu) & (y > yl)
    return m


def percentage_covered(uncovered, total) -> float:
    """src/FullSimulation.jl:557: 100 - (uncovered / total) * 100; total = 0 gives NaN, as Julia's
    0/0 does (x/0 with x > 0 cannot occur: uncovered <= total)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(100 - (np.float64(uncovered) / np.float64(total)) * 100)


class MadsParams(ctypes.Structure):
    """mac_mads_params (include/maxcover.h)."""
    _fields_ = [("n_iter", ctypes.c_int64), ("ell0", ctypes.c_int32), ("ell_max", ctypes.c_int32),
                ("seed", ctypes.c_uint64)]


class MadsStats(ctypes.Structure):
    """mac_mads_stats (include/maxcover.h)."""
    _fields_ = [("f", ctypes.c_double), ("iterations", ctypes.c_int64),
                ("evaluations", ctypes.c_int64), ("status", ctypes.c_int32),
                ("feasible", ctypes.c_int32), ("seconds", ctypes.c_double),
                ("host_enqueue_s", ctypes.c_double), ("host_perm_s", ctypes.c_double),
                ("wait_s", ctypes.c_double), ("host_post_s", ctypes.c_double),
                ("feasible_evaluations", ctypes.c_int64), ("rejected_polls", ctypes.c_int64),
                ("successes", ctypes.c_int64), ("slot_fallbacks", ctypes.c_int64)]


MAC_POLL_XYR = 0
MAC_POLL_XY = 1
POLL_VARS = {"xyr": MAC_POLL_XYR, "xy": MAC_POLL_XY}


class MadsOpts(ctypes.Structure):
    """mac_mads_opts (include/maxcover.h): the native driver's poll kind (16 B, reserved = 0)."""
    _fields_ = [("poll_vars", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


def poll_vars_code(poll_vars) -> int:
    """MAC_POLL_XYR / MAC_POLL_XY from "xyr" / "xy" (ValueError otherwise)."""
    try:
        return POLL_VARS[poll_vars]
    except (KeyError, TypeError):
        raise ValueError(f"poll_vars must be 'xyr' or 'xy', not {poll_vars!r}") from None


class MadsMesh(ctypes.Structure):
    """mac_mads_mesh (include/maxcover.h): the native driver's per-variable granularity (16 B,
    reserved = 0). ``granularity``: 3N host doubles laid out as x, or null for 1.0 everywhere."""
    _fields_ = [("granularity", ctypes.POINTER(ctypes.c_double)), ("reserved", ctypes.c_int64)]


def mesh_granularity(granularity, three_n: int):
    """The granularity vector g of a MADS run over ``three_n`` variables (x_0.., y_0.., r_0..), or
    None (1.0 everywhere): ``granularity`` is None, a scalar, a pair (g_xy, g_r) or ``three_n``
    values. Every entry must be finite and > 0 (ValueError otherwise)."""
    if granularity is None:
        return None
    try:
        g = np.asarray(granularity, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"granularity must be a number, a pair (g_xy, g_r) or {three_n} numbers, "
                         f"not {granularity!r}") from None
    N = three_n // 3
    if g.ndim == 0:
        g = np.full(three_n, float(g))
    elif g.ndim == 1 and g.size == 2:
        g = np.concatenate([np.full(2 * N, g[0]), np.full(three_n - 2 * N, g[1])])
    elif g.ndim != 1 or g.size != three_n:
        raise ValueError(f"granularity must be a number, a pair (g_xy, g_r) or {three_n} numbers, "
                         f"not an array of shape {g.shape}")
    if not (np.isfinite(g).all() and (g > 0).all()):
        raise ValueError("granularity: every entry must be finite and > 0")
    return np.ascontiguousarray(g, dtype=np.float64)


class FireParams(ctypes.Structure):
    """mac_fire_params (include/maxcover.h)."""
    _fields_ = [("nx", ctypes.c_int64), ("ny", ctypes.c_int64), ("dx", ctypes.c_double),
                ("dy", ctypes.c_double), ("forest_density", ctypes.c_double),
                ("prob_spread", ctypes.c_double), ("wind_speed", ctypes.c_double),
                ("wind_direction", ctypes.c_double), ("ix0", ctypes.c_int64),
                ("ix1", ctypes.c_int64), ("iy0", ctypes.c_int64), ("iy1", ctypes.c_int64),
                ("seed", ctypes.c_uint64)]


class Cons(ctypes.Structure):
    """mac_cons (include/maxcover.h): the swarm constraints a poll applies on the device. d_sep:
    cons8's minimum horizontal spacing (<= 0 or NaN: off); zone_y, zone_r: cons7's altitude zone
    (y < zone_y needs r <= zone_r; either NaN: off)."""
    _fields_ = [("d_sep", ctypes.c_double), ("zone_y", ctypes.c_double), ("zone_r", ctypes.c_double)]


def make_cons(cons=None, d_sep: float | None = None, zone_y: float | None = None,
              zone_r: float | None = None) -> Cons | None:
    """A Cons from a Cons, a mapping / object with d_sep, zone_y, zone_r fields (missing: off), or
    the keyword values; None stays None (all constraints off)."""
    if isinstance(cons, Cons):
        return cons
    if cons is not None:
        get = cons.get if hasattr(cons, "get") else lambda k, d=None: getattr(cons, k, d)
        d_sep, zone_y, zone_r = get("d_sep"), get("zone_y"), get("zone_r")
    elif d_sep is None and zone_y is None and zone_r is None:
        return None
    nan = float("nan")
    return Cons(nan if d_sep is None else float(d_sep), nan if zone_y is None else float(zone_y),
                nan if zone_r is None else float(zone_r))


class Motion(ctypes.Structure):
    """mac_motion (include/maxcover.h): the target-motion constraints cons4 (cone_cos, with vel),
    cons5 (v_max) and cons6 (a_max, with speed_prev) around the previous target ``anchor``. A NaN
    scalar or a NULL array switches its constraint off. Built by make_motion, which keeps the arrays
    alive on the object."""
    _fields_ = [("anchor", ctypes.POINTER(ctypes.c_double)), ("vel", ctypes.POINTER(ctypes.c_double)),
                ("speed_prev", ctypes.POINTER(ctypes.c_double)), ("cone_cos", ctypes.c_double),
                ("v_max", ctypes.c_double), ("a_max", ctypes.c_double)]


def make_motion(motion=None, anchor=None, vel=None, speed_prev=None, cone_cos: float | None = None,
                v_max: float | None = None, a_max: float | None = None) -> Motion | None:
    """A Motion from a Motion, a mapping / object with anchor, vel, speed_prev, cone_cos, v_max,
    a_max fields (missing: off), or the keyword values; None stays None (all constraints off).
    anchor: 3N [x; y; R]; vel: 2N [vx; vy]; speed_prev: N."""
    if isinstance(motion, Motion):
        return motion
    if motion is not None:
        get = motion.get if hasattr(motion, "get") else lambda k, d=None: getattr(motion, k, d)
        anchor, vel, speed_prev = get("anchor"), get("vel"), get("speed_prev")
        cone_cos, v_max, a_max = get("cone_cos"), get("v_max"), get("a_max")
    elif anchor is None:
        return None
    nan = float("nan")
    keep = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
            for a in (anchor, vel, speed_prev)]
    if keep[0] is None:
        raise ValueError("a motion constraint needs its anchor")
    N, rem = divmod(keep[0].size, 3)
    if rem or (keep[1] is not None and keep[1].size != 2 * N) or \
            (keep[2] is not None and keep[2].size != N):
        raise ValueError("motion: anchor is 3N, vel 2N and speed_prev N values")
    dp = ctypes.POINTER(ctypes.c_double)
    m = Motion(*[a.ctypes.data_as(dp) if a is not None else None for a in keep],
               nan if cone_cos is None else float(cone_cos), nan if v_max is None else float(v_max),
               nan if a_max is None else float(a_max))
    m._keep = keep   # the arrays the pointers refer to
    m.n_uav = N
    return m


MAC_VERDICT_KINDS = 6
# kind q of a verdict, in bit order (MAC_REJ_CONS3 = 1 << 0, ...)
VERDICT_KINDS = ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")
MAC_REJ_CONS3, MAC_REJ_CONS8, MAC_REJ_CONS7 = 0x01, 0x02, 0x04
MAC_REJ_CONS4, MAC_REJ_CONS5, MAC_REJ_CONS6 = 0x08, 0x10, 0x20


class Verdict(ctypes.Structure):
    """mac_verdict (include/maxcover.h): what rejected one candidate (64 B). reasons: the OR of
    MAC_REJ_* over the constraints that are on and reject it; pairs: cons8's violating unordered
    pairs; n_uav[q] / first_uav[q]: the UAVs that violate kind q and the lowest of them (-1: none)."""
    _fields_ = [("reasons", ctypes.c_uint32), ("pairs", ctypes.c_int32),
                ("n_uav", ctypes.c_int32 * MAC_VERDICT_KINDS),
                ("first_uav", ctypes.c_int32 * MAC_VERDICT_KINDS), ("reserved", ctypes.c_int32 * 2)]


# the same 64 bytes as a numpy record (Context.cons_explain's and TDM_Constraints.explain's result)
VERDICT_DTYPE = np.dtype([("reasons", "<u4"), ("pairs", "<i4"), ("n_uav", "<i4", (MAC_VERDICT_KINDS,)),
                          ("first_uav", "<i4", (MAC_VERDICT_KINDS,)), ("reserved", "<i4", (2,))])


class Prog(ctypes.Structure):
    """mac_prog (include/maxcover.h): the progressive constraints (altitude excess). Bit j of
    member[i]: UAV i belongs to constraint j; limit[i]: its altitude limit; n_cons = J <= 32;
    h_max0: the barrier's first threshold (negative or NaN: the default). Built by make_prog, which
    keeps the arrays alive on the object."""
    _fields_ = [("member", ctypes.POINTER(ctypes.c_uint32)), ("limit", ctypes.POINTER(ctypes.c_double)),
                ("n_cons", ctypes.c_int32), ("reserved", ctypes.c_int32), ("h_max0", ctypes.c_double)]


class MadsProgStats(ctypes.Structure):
    """mac_mads_prog_stats (include/maxcover.h)."""
    _fields_ = [("has_feasible", ctypes.c_int32), ("has_infeasible", ctypes.c_int32),
                ("f_feasible", ctypes.c_double), ("f_infeasible", ctypes.c_double),
                ("h_infeasible", ctypes.c_double), ("h_max", ctypes.c_double),
                ("dominating", ctypes.c_int64), ("improving", ctypes.c_int64),
                ("unsuccessful", ctypes.c_int64), ("two_centre_polls", ctypes.c_int64),
                ("evaluated", ctypes.c_int64)]


class ProgPart(ctypes.Structure):
    """mac_prog_part (include/maxcover.h): the shard-partial record of one iteration of the
    progressive barrier. ``tag``: the 1-based iteration, bit 62 set when the loop ends there."""
    _fields_ = [("tag", ctypes.c_int64), ("evaluated", ctypes.c_int64),
                ("bestF_f", ctypes.c_double), ("bestF_g", ctypes.c_int64),
                ("dominates", ctypes.c_int64), ("h_below", ctypes.c_double),
                ("keep_f", ctypes.c_double), ("keep_h", ctypes.c_double), ("keep_g", ctypes.c_int64),
                ("drop_f", ctypes.c_double), ("drop_h", ctypes.c_double), ("drop_g", ctypes.c_int64)]

    def words(self) -> np.ndarray:
        """The record's 12 words as float64 (raw bits: what a gather exchanges)."""
        return np.frombuffer(bytes(self), dtype=np.float64).copy()

    @classmethod
    def from_words(cls, w) -> "ProgPart":
        return cls.from_buffer_copy(np.ascontiguousarray(w, dtype=np.float64).tobytes())

    def as_tuple(self):
        return tuple(getattr(self, k) for k, _ in self._fields_)


PROG_TAG_DONE = 1 << 62


def prog_merge(parts) -> ProgPart:
    """mac_prog_merge: the records of one iteration (ProgPart, or 12 float64 words each) merged into one;
    exact, in any order. Unequal tags: MaxCoverError (MAC_E_INVAL). Needs no context."""
    ps = [p if isinstance(p, ProgPart) else ProgPart.from_words(p) for p in parts]
    arr = (ProgPart * max(len(ps), 1))(*ps)
    out = ProgPart()
    _check(load_library().mac_prog_merge(arr, len(ps), ctypes.byref(out)))
    return out


def make_prog(prog=None, member=None, limit=None, n_cons: int | None = None,
              h_max0: float | None = None) -> Prog | None:
    """A Prog from a Prog, a mapping / object with member, limit, n_cons (and h_max0) fields (e.g.
    TDM_Constraints.merge_mac_prog's mapping), or the keyword values; None stays None (no
    progressive constraint). A given ``h_max0`` overrides the mapping's; None: the default (-1)."""
    if isinstance(prog, Prog):
        if h_max0 is not None:
            prog.h_max0 = float(h_max0)
        return prog
    if prog is not None:
        get = prog.get if hasattr(prog, "get") else lambda k, d=None: getattr(prog, k, d)
        member, limit, n_cons = get("member"), get("limit"), get("n_cons")
        if h_max0 is None:
            h_max0 = get("h_max0")
    elif member is None and limit is None and n_cons is None:
        return None
    mem = None if member is None else np.ascontiguousarray(np.asarray(member).ravel(), dtype=np.uint32)
    lim = None if limit is None else np.ascontiguousarray(np.asarray(limit, dtype=np.float64).ravel())
    if mem is not None and lim is not None and mem.size != lim.size:
        raise ValueError("prog: member and limit hold N values each")
    p = Prog(mem.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if mem is not None else None,
             lim.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if lim is not None else None,
             0 if n_cons is None else int(n_cons), 0, -1.0 if h_max0 is None else float(h_max0))
    p._keep = (mem, lim)   # the arrays the pointers refer to
    p.n_uav = mem.size if mem is not None else (lim.size if lim is not None else 0)
    return p


def motion_thresholds(speed_prev: float, a_max: float) -> tuple[float, float]:
    """mac_motion_thresholds: cons6 for one UAV as (q_hi, q_lo): infeasible iff q3 > q_hi or
    q3 <= q_lo, with q3 the squared 3-D move."""
    hi, lo = ctypes.c_double(), ctypes.c_double()
    load_library().mac_motion_thresholds(float(speed_prev), float(a_max), ctypes.byref(hi),
                                         ctypes.byref(lo))
    return hi.value, lo.value


def _opt(s):
    return ctypes.byref(s) if s is not None else None


class MaxCoverError(RuntimeError):
    """Non-zero status from libmaxcover (message from mac_last_error)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"libmaxcover error {code}: {msg}")
        self.code = code


class InexactError(MaxCoverError, ValueError):
    """Julia's InexactError from Int(length(circles)/3) (src/AreaCoverageCalculation.jl:65)."""


_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64

_lib = None
_lib_lock = threading.Lock()


def _declare(L: ctypes.CDLL) -> None:
    sig = {
        "mac_last_error": ([], ctypes.c_char_p),
        "mac_version": ([], ctypes.c_char_p),
        "mac_device_count": ([ctypes.POINTER(_i32)], _i32),
        "mac_ctx_create": ([ctypes.POINTER(_vp), _i32], _i32),
        "mac_ctx_destroy": ([_vp], None),
        "mac_set_option": ([_vp, _i32, _i64], _i32),
        "mac_set_points_f64": ([_vp, _dp, _dp, _dp, _i64], _i32),
        "mac_set_points_records_f64": ([_vp, _dp, _i64, _i64], _i32),
        "mac_set_points_dev_f64": ([_vp, _vp, _vp, _vp, _i64], _i32),
        "mac_num_points": ([_vp, _i64p], _i32),
        "mac_get_points_f64": ([_vp, _dp, _dp, _dp], _i32),
        "mac_remove_covered_f64": ([_vp, _dp, _i64, _i64p, _i64p], _i32),
        "mac_covered_flags_f64": ([_vp, _dp, _i64, _u8p], _i32),
        "mac_area_f64": ([_vp, _dp, _i64, _dp], _i32),
        "mac_area_batch_f64": ([_vp, _dp, _i64, _i64, _dp], _i32),
        "mac_objective_batch_f64": ([_vp, _dp, _i64, _i64, _dp, ctypes.c_double, _dp], _i32),
        "mac_poll_best_f64": ([_vp, _dp, _i64, _i64, _dp, ctypes.c_double, _dp, _dp,
                               ctypes.c_double, _dp, _dp, _i64p], _i32),
        "mac_area_batch_dev_f64": ([_vp, _vp, _i64, _i64, _vp, _vp], _i32),
        "mac_area_by_disk_f64": ([_vp, _dp, _i64, _dp, _dp, _dp], _i32),
        "mac_area_by_disk_batch_f64": ([_vp, _dp, _i64, _i64, _dp, _dp, _dp], _i32),
        "mac_area_by_disk_dev_f64": ([_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp], _i32),
        "mac_poll_best_dev_f64": ([_vp, _vp, _i64, _i64, _vp, ctypes.c_double, _vp, _vp,
                                   ctypes.c_double, _i64, _vp, _vp, _vp], _i32),
        "mac_cons_mask_f64": ([_vp, _dp, _i64, _i64, ctypes.POINTER(Cons), _u8p], _i32),
        "mac_cons_mask_dev_f64": ([_vp, _vp, _i64, _i64, ctypes.POINTER(Cons), _vp, _vp], _i32),
        "mac_poll_best_cons_f64": ([_vp, _dp, _i64, _i64, _dp, ctypes.c_double, _dp, _dp,
                                    ctypes.c_double, _dp, _dp, _i64p, ctypes.POINTER(Cons)], _i32),
        "mac_poll_best_cons_dev_f64": ([_vp, _vp, _i64, _i64, _vp, ctypes.c_double, _vp, _vp,
                                        ctypes.c_double, _i64, _vp, _vp, _vp,
                                        ctypes.POINTER(Cons)], _i32),
        "mac_best_fetch": ([_vp, _vp, _vp, _dp, _i64p], _i32),
        "mac_best_reduce_dev": ([_vp, _vp, _i32, _vp, _vp], _i32),
        "mac_comm_unique_id": ([ctypes.c_char_p, _vp], _i32),
        "mac_comm_init": ([_vp, ctypes.c_char_p, _vp, _i32, _i32], _i32),
        "mac_poll_exchange": ([_vp, _vp, _vp, _vp, _dp, _i64p], _i32),
        "mac_exchange_records": ([_vp, _vp, _i32, _vp, _vp], _i32),
        "mac_poll_basis_f64": ([_vp, _dp, _i64, ctypes.POINTER(ctypes.c_int16),
                                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                ctypes.c_double, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                _dp, _dp, _i64p], _i32),
        "mac_poll_arm_dev_f64": ([_vp, _vp, _i64, _i64, _vp, ctypes.c_double, _vp, _vp,
                                  ctypes.c_double, _i64, _vp, _vp, _vp,
                                  ctypes.POINTER(ctypes.c_uint64)], _i32),
        "mac_poll_fire": ([_vp, ctypes.c_uint64], _i32),
        "mac_cover_threshold": ([ctypes.c_double], ctypes.c_double),
        "mac_profile_read": ([_vp, _dp, _i64p, _i64p, ctypes.POINTER(_i32), _i32], _i32),
        "mac_profile_split": ([_vp, _dp, _dp, _dp, _i64p], _i32),
        "mac_profile_kernels": ([_vp, _dp, _i64p, _i32], _i32),
        "mac_profile_fused": ([_vp, _i64p, _i64p, _i64p, _i32], _i32),
        "mac_diag_poll_report": ([_vp, ctypes.POINTER(_i32), _i32, ctypes.POINTER(_i32), _i32], _i32),
        "mac_append_points_f64": ([_vp, _dp, _dp, _dp, _i64], _i32),
        "mac_mads_run": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                          ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats)], _i32),
        "mac_mads_run_cons": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                               ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats),
                               ctypes.POINTER(Cons)], _i32),
        "mac_mads_begin_cons": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                 ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp),
                                 ctypes.POINTER(Cons)], _i32),
        "mac_mads_run_opts": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                               ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats),
                               ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts)], _i32),
        "mac_mads_begin_opts": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                 ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp),
                                 ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts)], _i32),
        "mac_cons_mask_motion_f64": ([_vp, _dp, _i64, _i64, ctypes.POINTER(Cons), _u8p,
                                      ctypes.POINTER(Motion)], _i32),
        "mac_poll_best_motion_f64": ([_vp, _dp, _i64, _i64, _dp, ctypes.c_double, _dp, _dp,
                                      ctypes.c_double, _dp, _dp, _i64p, ctypes.POINTER(Cons),
                                      ctypes.POINTER(Motion)], _i32),
        "mac_motion_thresholds": ([ctypes.c_double, ctypes.c_double, _dp, _dp], None),
        "mac_cons_explain_f64": ([_vp, _dp, _i64, _i64, _dp, _dp, ctypes.c_double, ctypes.POINTER(Cons),
                                  ctypes.POINTER(Motion), ctypes.POINTER(Verdict)], _i32),
        "mac_verdict_read": ([_vp, _i64p, _i64p, _i64p, _i64p, _i32], _i32),
        "mac_mads_run_motion": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                 ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats),
                                 ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts),
                                 ctypes.POINTER(Motion)], _i32),
        "mac_mads_begin_motion": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                   ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp),
                                   ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts),
                                   ctypes.POINTER(Motion)], _i32),
        "mac_mads_run_mesh": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                               ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats),
                               ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts),
                               ctypes.POINTER(Motion), ctypes.POINTER(MadsMesh)], _i32),
        "mac_mads_begin_mesh": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                 ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp),
                                 ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts),
                                 ctypes.POINTER(Motion), ctypes.POINTER(MadsMesh)], _i32),
        "mac_append_points_dev_f64": ([_vp, _vp, _vp, _vp, _i64], _i32),
        "mac_fire_last_error": ([], ctypes.c_char_p),
        "mac_fire_thresholds": ([ctypes.POINTER(FireParams), _dp], None),
        "mac_fire_create": ([ctypes.POINTER(_vp), _i32, ctypes.POINTER(FireParams)], _i32),
        "mac_fire_destroy": ([_vp], None),
        "mac_fire_initial_points": ([_vp, _dp, _i64, _i64p], _i32),
        "mac_fire_step": ([_vp, _vp, _i64p], _i32),
        "mac_fire_last_points": ([_vp, _dp, _i64, _i64p], _i32),
        "mac_fire_get_grid": ([_vp, _u8p], _i32),
        "mac_fire_set_grid": ([_vp, _u8p], _i32),
        "mac_mads_begin": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                            ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp)], _i32),
        "mac_prog_h_f64": ([_vp, _dp, _i64, _i64, ctypes.POINTER(Prog), _dp], _i32),
        "mac_mads_run_prog": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                               ctypes.POINTER(MadsParams), _dp, ctypes.POINTER(MadsStats),
                               ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts), ctypes.POINTER(Motion),
                               ctypes.POINTER(MadsMesh), ctypes.POINTER(Prog), _dp,
                               ctypes.POINTER(MadsProgStats)], _i32),
        "mac_mads_begin_prog": ([_vp, _dp, _i64, _dp, ctypes.c_double, _dp, _dp, ctypes.c_double,
                                 ctypes.POINTER(MadsParams), _i64, _i64, ctypes.POINTER(_vp),
                                 ctypes.POINTER(Cons), ctypes.POINTER(MadsOpts),
                                 ctypes.POINTER(Motion), ctypes.POINTER(MadsMesh), ctypes.POINTER(Prog)], _i32),
        "mac_mads_poll_prog": ([_vp, _i32, ctypes.POINTER(_i32), ctypes.POINTER(ProgPart)], _i32),
        "mac_prog_merge": ([ctypes.POINTER(ProgPart), _i32, ctypes.POINTER(ProgPart)], _i32),
        "mac_mads_advance_prog": ([_vp, ctypes.POINTER(ProgPart), ctypes.POINTER(_i32),
                                   ctypes.POINTER(_i32)], _i32),
        "mac_mads_result_prog": ([_vp, _dp, _dp, ctypes.POINTER(MadsStats),
                                  ctypes.POINTER(MadsProgStats)], _i32),
        "mac_mads_poll": ([_vp, ctypes.POINTER(_i32), _dp, _i64p], _i32),
        "mac_mads_update": ([_vp, ctypes.c_double, _i64], _i32),
        "mac_mads_poll_ahead": ([_vp, _i32, ctypes.POINTER(_i32), _dp, _i64p, _i64p], _i32),
        "mac_mads_advance": ([_vp, ctypes.c_double, _i64, ctypes.POINTER(_i32)], _i32),
        "mac_mads_result": ([_vp, _dp, ctypes.POINTER(MadsStats)], _i32),
        "mac_mads_destroy": ([_vp], None),
        "mac_mads_best_buffer": ([_vp, _vp], _i32),
        "mac_set_regions": ([_vp, _dp, _dp, _dp, _dp, _i32, ctypes.c_double], _i32),
        "mac_regions_ingested": ([_vp, _i64p, _i64p], _i32),
        "mac_region_stats_f64": ([_vp, _dp, _i64, _i64p, _dp, _i64p, _dp, _i64p, _dp], _i32),
        "mac_set_points_f32": ([_vp, _fp, _fp, _fp, _i64], _i32),
        "mac_set_points_dev_f32": ([_vp, _vp, _vp, _vp, _i64], _i32),
        "mac_area_f32": ([_vp, _fp, _i64, _dp], _i32),
        "mac_area_batch_f32": ([_vp, _fp, _i64, _i64, _dp], _i32),
        "mac_poll_best_f32": ([_vp, _fp, _i64, _i64, _dp, ctypes.c_double, _fp, _dp,
                               ctypes.c_double, _dp, _dp, _i64p], _i32),
        "mac_poll_best_dev_f32": ([_vp, _vp, _i64, _i64, _vp, ctypes.c_double, _vp, _vp,
                                   ctypes.c_double, _i64, _vp, _vp, _vp], _i32),
    }
    for name, (args, res) in sig.items():
        # (an older build lacks the newer symbols: bound as far as it has them, so A/B tools can
        # load it; tests/test_abi.py checks that the in-tree library exports every one)
        f = getattr(L, name, None)
        if f is None:
            continue
        f.argtypes = args
        f.restype = res


_loaded_before_torch = False


def _one_hip_runtime() -> None:
    """PyTorch-ROCm ships its own HIP and HSA runtimes, which its libraries load by file name. If
    libmaxcover.so (NEEDED libamdhip64.so.7) is loaded first, it binds the system runtime and a
    later torch import loads a second one in the same process, whose device initialisation fails
    ("No HIP GPUs are available"; measured on the MI355X box). With torch loaded first, libmaxcover
    shares torch's runtime: one context for torch tensors, streams, RCCL and the library.

    So a process that uses both must import torch first. The library does not
    import torch itself — a CPU-only user does not pay for it, and which runtime binds does not
    depend silently on whether torch is importable — unless MAXCOVER_TORCH_FIRST=1 asks for it.
    Whether torch was already loaded is recorded: `check_one_runtime` (called by dist.py before
    its device collectives) fails loudly instead of letting two runtimes meet."""
    global _loaded_before_torch
    import sys
    if "torch" not in sys.modules and os.environ.get("MAXCOVER_TORCH_FIRST") == "1":
        import torch  # noqa: F401
    _loaded_before_torch = "torch" not in sys.modules


def check_one_runtime() -> None:
    """Raise if libmaxcover was loaded before torch in this process (two HIP runtimes: torch's
    device work and the library's would not share a context; see _one_hip_runtime)."""
    if _lib is not None and _loaded_before_torch:
        raise MaxCoverError(MAC_E_HIP, "libmaxcover was loaded before torch: import torch before the "
                            "first libmaxcover call (one HIP runtime per process, INTEGRATION.md)")


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libmaxcover.so (raises MaxCoverError if absent: there is no fallback path)."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise MaxCoverError(MAC_E_HIP, f"{p} not built (run __graft_entry__.build())")
        _one_hip_runtime()
        try:
            L = ctypes.CDLL(p)
        except OSError as e:  # pragma: no cover - depends on the host
            raise MaxCoverError(MAC_E_HIP, f"cannot load {p}: {e}") from e
        _declare(L)
        if path is None:
            _lib = L
        return L


def _check(rc: int) -> None:
    if rc != MAC_OK:
        msg = load_library().mac_last_error().decode(errors="replace")
        if rc == MAC_E_SIZE:
            raise InexactError(rc, msg)
        raise MaxCoverError(rc, msg)


def version() -> str:
    return load_library().mac_version().decode()


def device_count() -> int:
    n = _i32()
    _check(load_library().mac_device_count(ctypes.byref(n)))
    return int(n.value)


def cover_threshold(r: float) -> float:
    return float(load_library().mac_cover_threshold(float(r)))


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_dp)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(_fp)


def _devptr(t) -> int:
    """Device address of a torch tensor / int / None."""
    if t is None:
        return 0
    if isinstance(t, int):
        return t
    return int(t.data_ptr())


def _stream(stream, device: int) -> int:
    """hipStream_t handle for a *_dev call. An int is a raw handle (0: HIP's null stream, the C
    ABI's NULL); a torch stream gives its handle; None follows torch's convention — the current
    torch stream of the context's device when this process has initialised torch's GPU side (so a
    poll is ordered after the torch ops that produced its inputs), else HIP's null stream."""
    if stream is None:
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_initialized():
            return int(torch.cuda.current_stream(device).cuda_stream)
        return 0
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


class Context:
    """One libmaxcover context = one GPU + one device-resident fire-point list."""

    def __init__(self, device: int = 0, algo: str = "auto", tile_points: int | None = None):
        L = load_library()
        h = _vp()
        _check(L.mac_ctx_create(ctypes.byref(h), int(device)))
        self._h = h
        self.device = int(device)
        self._L = L
        self._steppers = weakref.WeakSet()   # closed before the context (they use its device state)
        self._n_boxes = 0                    # high-interest boxes set (set_regions)
        self.set_algo(algo)
        if tile_points is not None:
            self.set_option(MAC_OPT_TILE_POINTS, int(tile_points))

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None):
            for st in list(getattr(self, "_steppers", ())):
                st.close()
            self._L.mac_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- options
    def set_option(self, option: int, value: int) -> None:
        _check(self._L.mac_set_option(self._h, int(option), int(value)))

    def set_shared(self, mode: str) -> None:
        """How the poll walk decides the entries two disks' regions share (MAC_OPT_SHARED):
        "auto" (default), "fp64" (the poll kernel's jobs) or "bits" (the bit-word kernel)."""
        self.set_option(MAC_OPT_SHARED, SHARED_MODES[mode])

    def set_chain(self, chain: str) -> None:
        """The poll chain (MAC_OPT_CHAIN): "auto" (default: the fused three-launch chain unless the
        lane's recent polls were crowded, scattered or off the packed-key grid), "five" (prep, index,
        set-up, walk, finalize) or "fused" (prep, fiw, fin2 whenever it applies)."""
        self.set_option(MAC_OPT_CHAIN, CHAINS[chain])

    def set_mesh_keys(self, on: bool = True) -> None:
        """How the native MADS driver's polls on a mesh (``mesh=`` of mads_run / mads_begin) key
        their disks (MAC_OPT_MESH_KEYS): off (default) by their offsets in metres, which pack only at
        integer granularities; on by the poll's signed integer draws, which pack at every granularity.
        Results are the same; read when a run or a stepper begins (a stepper keeps its mode)."""
        self.set_option(MAC_OPT_MESH_KEYS, MAC_KEYS_MESH if on else MAC_KEYS_VALUE)

    def set_verdicts(self, on: bool = True) -> None:
        """Whether the native MADS driver tallies what rejected the candidates of the polls it
        generates (MAC_OPT_VERDICTS; verdict_read). Read when a run or a stepper begins (a stepper
        keeps what it began with); results and statistics are the same either way. A run with
        ``prog=`` ignores it."""
        self.set_option(MAC_OPT_VERDICTS, 1 if on else 0)

    def verdict_read(self, reset: bool = True) -> dict:
        """mac_verdict_read: the driver's tally since the last reset, as ``dict(candidates,
        rejected_any, rejected_by={"cons3": .., "cons8": .., "cons7": .., "cons4": .., "cons5": ..,
        "cons6": ..}, polls)``. Synchronises the device."""
        c, a, p = _i64(), _i64(), _i64()
        by = (_i64 * MAC_VERDICT_KINDS)()
        _check(self._L.mac_verdict_read(self._h, ctypes.byref(c), ctypes.byref(a), by, ctypes.byref(p),
                                        1 if reset else 0))
        return {"candidates": int(c.value), "rejected_any": int(a.value),
                "rejected_by": {k: int(by[q]) for q, k in enumerate(VERDICT_KINDS)},
                "polls": int(p.value)}

    def set_algo(self, algo: str) -> None:
        if algo not in ALGOS:
            raise ValueError(f"algo must be one of {sorted(ALGOS)}")
        self.set_option(MAC_OPT_ALGO, ALGOS[algo])

    def profile(self, on: bool = True) -> None:
        self.set_option(MAC_OPT_PROFILE, 1 if on else 0)

    def profile_read(self, reset: bool = True):
        """(coverage-kernel ms summed over launches, launches, candidates evaluated, walk used
        by the last launch: 'scan' | 'tiled' | 'poll' | None)."""
        ms = ctypes.c_double()
        n = _i64()
        k = _i64()
        a = _i32()
        _check(self._L.mac_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(k),
                                        ctypes.byref(a), 1 if reset else 0))
        name = {MAC_ALGO_SCAN: "scan", MAC_ALGO_TILED: "tiled", MAC_ALGO_POLL: "poll"}.get(a.value)
        return ms.value, int(n.value), int(k.value), name

    def profile_split(self):
        """Poll chains since the last reset: (prep ms, walk ms, after-walk ms, polls), summed.
        Call before profile_read(reset=True)."""
        p1, p2, gap = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = _i64()
        _check(self._L.mac_profile_split(self._h, ctypes.byref(p1), ctypes.byref(p2),
                                         ctypes.byref(gap), ctypes.byref(n)))
        return p1.value, p2.value, gap.value, int(n.value)

    def profile_kernels(self):
        """Poll chains since the last reset, per launch role (mac_profile_kernels): {kernel name:
        (summed launch spans in ms, launches)}. Call before profile_read(reset=True)."""
        n = len(PROF_ROLES)
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        _check(self._L.mac_profile_kernels(self._h, ms, cnt, n))
        return {name: (ms[r], int(cnt[r])) for r, name in enumerate(PROF_ROLES)}

    def profile_fused(self, reset: bool = False) -> dict:
        """With profiling on, the fused chain's hint reports read so far (mac_profile_fused): reports,
        and the sum and the largest of hint word 1 (disks of a poll that took one position per
        candidate)."""
        r, s, m = _i64(), _i64(), _i64()
        _check(self._L.mac_profile_fused(self._h, ctypes.byref(r), ctypes.byref(s), ctypes.byref(m),
                                         1 if reset else 0))
        return {"reports": int(r.value), "ident_sum": int(s.value), "ident_max": int(m.value)}

    def poll_report(self, n_disks: int) -> dict:
        """What decided the shared entries of the context's most recent five-launch poll
        (mac_diag_poll_report; host only, synchronises the device): the walk that ran, the poll
        walk's counters by name (csrc/k_common.h kDc*) and the positions of each of its n_disks
        disks."""
        words = (_i32 * (1 + len(POLL_COUNTERS)))()
        uc = (_i32 * max(1, int(n_disks)))()
        _check(self._L.mac_diag_poll_report(self._h, words, len(words), uc, int(n_disks)))
        out = {"walk": {1: "poll", 2: "tiled"}.get(int(words[0])),
               "ucount": np.array(uc[:int(n_disks)], dtype=np.int64)}
        out.update({name: int(words[1 + q]) for q, name in enumerate(POLL_COUNTERS)})
        return out

    # -- point list
    def set_points(self, x, y, w) -> None:
        x, y, w = _f64(x), _f64(y), _f64(w)
        if not (x.shape == y.shape == w.shape) or x.ndim != 1:
            raise ValueError("x, y, w must be 1-D arrays of equal length")
        _check(self._L.mac_set_points_f64(self._h, _ptr(x), _ptr(y), _ptr(w), x.size))

    def set_points_f32(self, x, y, w) -> None:
        """fp32 SoA arrays (mac_set_points_f32): widened exactly to the fp64 list."""
        x, y, w = _f32(x), _f32(y), _f32(w)
        if not (x.shape == y.shape == w.shape) or x.ndim != 1:
            raise ValueError("x, y, w must be 1-D arrays of equal length")
        _check(self._L.mac_set_points_f32(self._h, _fptr(x), _fptr(y), _fptr(w), x.size))

    def set_points_device_f32(self, x, y, w, M: int | None = None) -> None:
        """x, y, w: torch float32 tensors on this context's device (widened copies)."""
        n = int(M if M is not None else x.numel())
        _check(self._L.mac_set_points_dev_f32(self._h, _devptr(x), _devptr(y), _devptr(w), n))

    def set_points_records(self, rec) -> None:
        r = _f64(rec)
        if r.ndim == 1:
            r = r.reshape(-1, 5)
        if r.ndim != 2 or (r.shape[0] and r.shape[1] < 4):
            raise ValueError("records must be M x >=4 ([x, y, area, importance, covered])")
        _check(self._L.mac_set_points_records_f64(self._h, _ptr(r), r.shape[0],
                                                  r.shape[1] if r.shape[0] else 5))

    def set_points_device(self, x, y, w, M: int | None = None) -> None:
        """x, y, w: torch float64 tensors on this context's device (copied)."""
        n = int(M if M is not None else x.numel())
        _check(self._L.mac_set_points_dev_f64(self._h, _devptr(x), _devptr(y), _devptr(w), n))

    def append_points(self, x, y, w) -> None:
        """update_POI (src/CellFunctions.jl:59-79): entries appended at the end of the list."""
        x, y, w = _f64(x), _f64(y), _f64(w)
        if not (x.size == y.size == w.size):
            raise ValueError("x, y, w lengths differ")
        _check(self._L.mac_append_points_f64(self._h, _ptr(x), _ptr(y), _ptr(w), x.size))

    def append_points_device(self, x, y, w, m: int | None = None) -> None:
        m = int(x.numel() if m is None else m)
        _check(self._L.mac_append_points_dev_f64(self._h, _devptr(x), _devptr(y), _devptr(w), m))

    @property
    def num_points(self) -> int:
        m = _i64()
        _check(self._L.mac_num_points(self._h, ctypes.byref(m)))
        return int(m.value)

    def get_points(self):
        M = self.num_points
        x = np.empty(M)
        y = np.empty(M)
        w = np.empty(M)
        _check(self._L.mac_get_points_f64(self._h, _ptr(x), _ptr(y), _ptr(w)))
        return x, y, w

    def covered_flags(self, circles) -> np.ndarray:
        c = _f64(circles)
        out = np.zeros(max(self.num_points, 1), dtype=np.uint8)
        _check(self._L.mac_covered_flags_f64(self._h, _ptr(c), c.size,
                                             out.ctypes.data_as(_u8p)))
        return out[: self.num_points].astype(bool)

    def remove_covered(self, circles) -> np.ndarray:
        """rmvCoveredPOI on the device list; returns the kept original indices (list order)."""
        c = _f64(circles)
        M = self.num_points
        kept = np.zeros(max(M, 1), dtype=np.int64)
        m = _i64()
        _check(self._L.mac_remove_covered_f64(self._h, _ptr(c), c.size,
                                              kept.ctypes.data_as(_i64p), ctypes.byref(m)))
        return kept[: m.value].copy()

    # -- high-interest regions
    def set_regions(self, x_LB, x_UB, y_LB, y_UB, w_high: float = float("nan")) -> None:
        """mac_set_regions: the boxes (x_LB[b], x_UB[b]) x (y_LB[b], y_UB[b]) (the reference's
        vectors, src/FullSimulation.jl:751-754). While they are set, every entry arriving in the
        list strictly inside any box gets weight ``w_high`` (NaN: weights left alone) and is
        counted (regions_ingested). Zeroes the counters; entries already in the list keep their
        weights. No boxes: clear_regions()."""
        b = [_f64(np.atleast_1d(v)).ravel() for v in (x_LB, x_UB, y_LB, y_UB)]
        n = b[0].size
        if any(v.size != n for v in b):
            raise ValueError("x_LB, x_UB, y_LB, y_UB must have equal lengths")
        _check(self._L.mac_set_regions(self._h, _ptr(b[0]), _ptr(b[1]), _ptr(b[2]), _ptr(b[3]), n,
                                       float(w_high)))
        self._n_boxes = n

    def clear_regions(self) -> None:
        _check(self._L.mac_set_regions(self._h, None, None, None, None, 0, float("nan")))
        self._n_boxes = 0

    def regions_ingested(self):
        """mac_regions_ingested: (per-box counts, union count) of the entries that arrived inside
        the boxes since set_points / set_regions last reset the counters."""
        n = self._n_boxes
        box = np.zeros(max(n, 1), dtype=np.int64)
        tot = _i64()
        _check(self._L.mac_regions_ingested(self._h, box.ctypes.data_as(_i64p), ctypes.byref(tot)))
        return box[:n].copy(), int(tot.value)

    def region_stats(self, circles=None) -> dict:
        """mac_region_stats_f64 on the current list: ``box_count`` / ``box_weight`` per box,
        ``any_count`` / ``any_weight`` for the union of the boxes (each entry once) and, with
        ``circles`` ([x; y; r]), ``covered_count`` / ``covered_weight``: the union's entries covered
        by at least one disk (0 without circles)."""
        n = self._n_boxes
        c = _f64(() if circles is None else circles).ravel()
        bc = np.zeros(max(n, 1), dtype=np.int64)
        bw = np.zeros(max(n, 1))
        ac, cc = _i64(), _i64()
        aw, cw = ctypes.c_double(), ctypes.c_double()
        _check(self._L.mac_region_stats_f64(self._h, _ptr(c) if c.size else None, c.size,
                                            bc.ctypes.data_as(_i64p), _ptr(bw), ctypes.byref(ac),
                                            ctypes.byref(aw), ctypes.byref(cc), ctypes.byref(cw)))
        return dict(box_count=bc[:n].copy(), box_weight=bw[:n].copy(), any_count=int(ac.value),
                    any_weight=aw.value, covered_count=int(cc.value), covered_weight=cw.value)

    # -- objective
    def area(self, circles) -> float:
        c = _f64(circles)
        out = ctypes.c_double()
        _check(self._L.mac_area_f64(self._h, _ptr(c), c.size, ctypes.byref(out)))
        return out.value

    def area_batch(self, cands) -> np.ndarray:
        """cands: K x 3N (row k = candidate k, i.e. the 3N x K column-major matrix)."""
        c = _f64(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        out = np.empty(K)
        _check(self._L.mac_area_batch_f64(self._h, _ptr(c), three_n, K, _ptr(out)))
        return out

    def area_by_disk(self, circles):
        """mac_area_by_disk_f64: (owned[N], exclusive[N], area) of one candidate. owned[i] is the
        weight of the entries whose first covering disk in index order is i (they sum to the area),
        exclusive[i] the weight disk i alone covers (area(all) - area(all but i))."""
        c = _f64(circles).ravel()
        N = c.size // 3
        owned = np.zeros(N)
        excl = np.zeros(N)
        out = ctypes.c_double()
        _check(self._L.mac_area_by_disk_f64(self._h, _ptr(c), c.size, _ptr(owned), _ptr(excl),
                                            ctypes.byref(out)))
        return owned, excl, out.value

    def area_by_disk_batch(self, cands):
        """mac_area_by_disk_batch_f64. cands: K x 3N (row k = candidate k). Returns
        (owned[K, N], exclusive[K, N], area[K])."""
        c = _f64(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        N = three_n // 3
        owned = np.zeros((K, N))
        excl = np.zeros((K, N))
        area = np.zeros(K)
        _check(self._L.mac_area_by_disk_batch_f64(self._h, _ptr(c), three_n, K, _ptr(owned),
                                                  _ptr(excl), _ptr(area)))
        return owned, excl, area

    def area_by_disk_dev(self, d_cands, three_n: int, K: int, d_owned, d_exclusive, d_area,
                         stream=None) -> None:
        """mac_area_by_disk_dev_f64: device pointers (torch float64 tensors / ints; any of the three
        outputs may be None, not all), ordered on `stream`; returns after enqueueing."""
        _check(self._L.mac_area_by_disk_dev_f64(self._h, _devptr(d_cands), int(three_n), int(K),
                                                _devptr(d_owned), _devptr(d_exclusive),
                                                _devptr(d_area), _stream(stream, self.device)))

    def objective_batch(self, cands, r_max, penalty: float = 1e5) -> np.ndarray:
        c = _f64(cands)
        K, three_n = c.shape
        rm = _f64(r_max)
        out = np.empty(K)
        _check(self._L.mac_objective_batch_f64(self._h, _ptr(c), three_n, K, _ptr(rm),
                                               float(penalty), _ptr(out)))
        return out

    def cons_mask(self, cands, cons, motion=None) -> np.ndarray:
        """mac_cons_mask_f64: the feasibility of each candidate (K x 3N rows) under ``cons`` (a Cons,
        or anything make_cons takes; None: all feasible), as a bool array. No point list needed.
        ``motion`` (a Motion, or anything make_motion takes): the target-motion constraints as well
        (mac_cons_mask_motion_f64)."""
        c = _f64(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        out = np.zeros(max(K, 1), dtype=np.uint8)
        cs = make_cons(cons)
        if motion is not None:
            mo = make_motion(motion)
            _check(self._L.mac_cons_mask_motion_f64(self._h, _ptr(c), three_n, K, _opt(cs),
                                                    out.ctypes.data_as(_u8p), _opt(mo)))
            return out[:K].astype(bool)
        _check(self._L.mac_cons_mask_f64(self._h, _ptr(c), three_n, K,
                                         ctypes.byref(cs) if cs is not None else None,
                                         out.ctypes.data_as(_u8p)))
        return out[:K].astype(bool)

    def cons_explain(self, cands, cons=None, motion=None, prev=None, d_lim=None,
                     tan_half_fov: float = 1.0) -> np.ndarray:
        """mac_cons_explain_f64: what rejects each candidate (K x 3N rows), one VERDICT_DTYPE record
        each: every constraint that is on (``cons``, ``motion`` as cons_mask takes them; cons3 through
        ``prev`` / ``d_lim`` / ``tan_half_fov`` as poll_best takes them) is evaluated for every
        candidate, none short-circuits another. TDM_Constraints.explain is the host mirror. No point
        list needed."""
        c = _f64(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        out = np.zeros(max(K, 1), dtype=VERDICT_DTYPE)
        cs = make_cons(cons)
        mo = make_motion(motion)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        _check(self._L.mac_cons_explain_f64(
            self._h, _ptr(c), three_n, K, _ptr(pv) if pv is not None else None,
            _ptr(dl) if dl is not None else None, float(tan_half_fov), _opt(cs), _opt(mo),
            out.ctypes.data_as(ctypes.POINTER(Verdict))))
        return out[:K]

    def prog_h(self, cands, prog) -> np.ndarray:
        """mac_prog_h_f64: the progressive constraints' violation h of each candidate (K x 3N rows)
        under ``prog`` (a Prog, or anything make_prog takes; None: all 0.0). No point list needed."""
        c = _f64(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        out = np.zeros(max(K, 1))
        pg = make_prog(prog)
        if pg is not None and pg.n_cons > 0 and pg.n_uav != three_n // 3:
            raise ValueError("prog: member and limit hold N values each")
        _check(self._L.mac_prog_h_f64(self._h, _ptr(c), three_n, K, _opt(pg), _ptr(out)))
        return out[:K]

    def cons_mask_dev(self, d_cands, three_n: int, K: int, cons, d_feasible, stream=None) -> None:
        """mac_cons_mask_dev_f64: device pointers (d_feasible: K uint8), ordered on ``stream``."""
        cs = make_cons(cons)
        _check(self._L.mac_cons_mask_dev_f64(self._h, _devptr(d_cands), int(three_n), int(K),
                                             ctypes.byref(cs) if cs is not None else None,
                                             _devptr(d_feasible), _stream(stream, self.device)))

    def poll_best(self, cands, r_max, penalty: float = 1e5, prev=None, d_lim=None,
                  tan_half_fov: float = 1.0, want_all: bool = False, cons=None, motion=None):
        """Returns (best_obj, best_idx[, objectives]); best_idx = -1 if none feasible. ``cons`` (a
        Cons, or anything make_cons takes): the swarm constraints applied on the device
        (mac_poll_best_cons_f64); None keeps the plain call. ``motion`` (a Motion, or anything
        make_motion takes): the target-motion constraints as well (mac_poll_best_motion_f64)."""
        c = _f64(cands)
        K, three_n = c.shape
        rm = _f64(r_max)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        objs = np.empty(K) if want_all else None
        bo = ctypes.c_double()
        bi = _i64()
        args = (self._h, _ptr(c), three_n, K, _ptr(rm), float(penalty),
                _ptr(pv) if pv is not None else None, _ptr(dl) if dl is not None else None,
                float(tan_half_fov), _ptr(objs) if objs is not None else None,
                ctypes.byref(bo), ctypes.byref(bi))
        if motion is not None:
            cs, mo = make_cons(cons), make_motion(motion)
            _check(self._L.mac_poll_best_motion_f64(*args, _opt(cs), _opt(mo)))
        elif cons is None:
            _check(self._L.mac_poll_best_f64(*args))
        else:
            cs = make_cons(cons)
            _check(self._L.mac_poll_best_cons_f64(*args, ctypes.byref(cs)))
        if want_all:
            return bo.value, int(bi.value), objs
        return bo.value, int(bi.value)

    def poll_basis(self, x_inc, L, rp, cp, delta: float, r_max, penalty: float = 1e5, prev=None,
                   d_lim=None, tan_half_fov: float = 1.0, want_all: bool = False):
        """mac_poll_basis_f64: the 2n-candidate poll x +- delta * B[:, k], B = L[rp][:, cp],
        expanded on the device. L: n x n lower-triangular integers (|L| < 2^15; its lower triangle
        is packed here) or the packed int16 triangle itself. Returns (best_obj, best_idx[, objs])."""
        x = _f64(x_inc)
        n = x.size
        Lp = np.asarray(L)
        if Lp.ndim == 2:
            if Lp.shape != (n, n):
                raise ValueError("L must be n x n")
            if np.abs(Lp).max(initial=0) > 32767:
                raise ValueError("|L| must fit int16")
            Lp = Lp[np.tril_indices(n)]
        tri = np.ascontiguousarray(Lp, dtype=np.int16)
        if tri.size != n * (n + 1) // 2:
            raise ValueError("packed L must hold n(n+1)/2 entries")
        r = np.ascontiguousarray(rp, dtype=np.int32)
        c = np.ascontiguousarray(cp, dtype=np.int32)
        if r.size != n or c.size != n:
            raise ValueError("rp / cp must hold n entries")
        rm = _f64(r_max)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        objs = np.empty(2 * n) if want_all else None
        bo = ctypes.c_double()
        bi = _i64()
        _check(self._L.mac_poll_basis_f64(
            self._h, _ptr(x), n, tri.ctypes.data_as(ctypes.POINTER(ctypes.c_int16)),
            r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            float(delta), _ptr(rm), float(penalty), _ptr(pv) if pv is not None else None,
            _ptr(dl) if dl is not None else None, float(tan_half_fov),
            _ptr(objs) if objs is not None else None, ctypes.byref(bo), ctypes.byref(bi)))
        if want_all:
            return bo.value, int(bi.value), objs
        return bo.value, int(bi.value)

    # -- fp32 candidates (*_f32: widened exactly on the device, fp64 decisions)
    def area_f32(self, circles) -> float:
        c = _f32(circles)
        out = ctypes.c_double()
        _check(self._L.mac_area_f32(self._h, _fptr(c), c.size, ctypes.byref(out)))
        return out.value

    def area_batch_f32(self, cands) -> np.ndarray:
        c = _f32(cands)
        if c.ndim != 2:
            raise ValueError("cands must be K x 3N")
        K, three_n = c.shape
        out = np.empty(K)
        _check(self._L.mac_area_batch_f32(self._h, _fptr(c), three_n, K, _ptr(out)))
        return out

    def poll_best_f32(self, cands, r_max, penalty: float = 1e5, prev=None, d_lim=None,
                      tan_half_fov: float = 1.0, want_all: bool = False):
        c = _f32(cands)
        K, three_n = c.shape
        rm = _f64(r_max)
        pv = _f32(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        objs = np.empty(K) if want_all else None
        bo = ctypes.c_double()
        bi = _i64()
        _check(self._L.mac_poll_best_f32(
            self._h, _fptr(c), three_n, K, _ptr(rm), float(penalty),
            _fptr(pv) if pv is not None else None, _ptr(dl) if dl is not None else None,
            float(tan_half_fov), _ptr(objs) if objs is not None else None,
            ctypes.byref(bo), ctypes.byref(bi)))
        if want_all:
            return bo.value, int(bi.value), objs
        return bo.value, int(bi.value)

    def poll_best_dev_f32(self, d_cands, three_n: int, K: int, d_rmax, d_best,
                          penalty: float = 1e5, d_prev=None, d_dlim=None, tan_half_fov: float = 1.0,
                          idx_base: int = 0, d_obj=None, stream=None) -> None:
        _check(self._L.mac_poll_best_dev_f32(
            self._h, _devptr(d_cands), int(three_n), int(K), _devptr(d_rmax), float(penalty),
            _devptr(d_prev), _devptr(d_dlim), float(tan_half_fov), int(idx_base),
            _devptr(d_obj), _devptr(d_best), _stream(stream, self.device)))

    # -- native MADS driver
    def mads_run(self, x0, r_max, penalty: float = 1e5, prev=None, d_lim=None,
                 tan_half_fov: float = 1.0, n_iter: int = 100, ell0: int = 2, ell_max: int = 6,
                 seed: int = 20250216, cons=None, poll_vars: str = "xyr", motion=None,
                 granularity=None, prog=None, h_max0=None):
        """mac_mads_run: the whole MADS loop in libmaxcover (candidates generated on the device).
        ``cons`` (a Cons, or anything make_cons takes, e.g. TDM_Constraints.merge_mac_cons's
        mapping): the swarm constraints every poll applies on the device (mac_mads_run_cons); None
        keeps the plain call. ``poll_vars``: "xyr" polls every variable (the calls above), "xy"
        x and y only with the radii held (mac_mads_run_opts, MAC_POLL_XY). ``motion`` (a Motion, or
        anything make_motion takes): the target-motion constraints on every poll
        (mac_mads_run_motion). ``granularity``: None, a scalar, a pair (g_xy, g_r) or 3N values laid
        out as x0 (mesh_granularity): variable v steps by g[v] times the basis's integers
        (mac_mads_run_mesh); None keeps the calls above. ``prog`` (a Prog, or anything make_prog
        takes, e.g. TDM_Constraints.merge_mac_prog's mapping): progressive constraints under the
        progressive barrier, first threshold ``h_max0`` (mac_mads_run_prog); the stats then gain
        mac_mads_prog_stats' fields and ``x_infeasible`` (the infeasible incumbent or None), and
        x is the feasible incumbent when there is one. None keeps the calls above.
        Returns (x, stats dict)."""
        pvars = poll_vars_code(poll_vars)
        x = _f64(x0)
        g = mesh_granularity(granularity, x.size)
        rm = _f64(r_max)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        out = np.empty_like(x)
        prm = MadsParams(int(n_iter), int(ell0), int(ell_max), int(seed) & (2**64 - 1))
        st = MadsStats()
        args = (self._h, _ptr(x), x.size, _ptr(rm), float(penalty),
                _ptr(pv) if pv is not None else None, _ptr(dl) if dl is not None else None,
                float(tan_half_fov), ctypes.byref(prm), _ptr(out), ctypes.byref(st))
        cs = make_cons(cons)
        pg = make_prog(prog, h_max0=h_max0)
        if pg is not None:
            if pg.n_cons > 0 and pg.n_uav != x.size // 3:
                raise ValueError("prog: member and limit hold N values each")
            op, mo = MadsOpts(pvars), make_motion(motion) if motion is not None else None
            mesh = MadsMesh(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0) if g is not None else None
            xi = np.full_like(x, np.nan)
            ps = MadsProgStats()
            _check(self._L.mac_mads_run_prog(*args, _opt(cs), ctypes.byref(op), _opt(mo), _opt(mesh),
                                             ctypes.byref(pg), _ptr(xi), ctypes.byref(ps)))
            stats = {k: getattr(st, k) for k, _ in MadsStats._fields_}
            if pg.n_cons > 0:
                stats.update({k: getattr(ps, k) for k, _ in MadsProgStats._fields_})
                stats["x_infeasible"] = xi if ps.has_infeasible else None
            return out, stats
        if g is not None:
            op, mo = MadsOpts(pvars), make_motion(motion) if motion is not None else None
            mesh = MadsMesh(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0)
            _check(self._L.mac_mads_run_mesh(*args, _opt(cs), ctypes.byref(op), _opt(mo),
                                             ctypes.byref(mesh)))
        elif motion is not None:
            op, mo = MadsOpts(pvars), make_motion(motion)
            _check(self._L.mac_mads_run_motion(*args, _opt(cs), ctypes.byref(op), _opt(mo)))
        elif pvars != MAC_POLL_XYR:
            op = MadsOpts(pvars)
            _check(self._L.mac_mads_run_opts(*args, ctypes.byref(cs) if cs is not None else None,
                                             ctypes.byref(op)))
        elif cs is None:
            _check(self._L.mac_mads_run(*args))
        else:
            _check(self._L.mac_mads_run_cons(*args, ctypes.byref(cs)))
        return out, {k: getattr(st, k) for k, _ in MadsStats._fields_}

    def mads_stepper(self, x0, r_max, penalty: float = 1e5, prev=None, d_lim=None,
                     tan_half_fov: float = 1.0, n_iter: int = 100, ell0: int = 2,
                     ell_max: int = 6, seed: int = 20250216, shard=None,
                     cons=None, poll_vars: str = "xyr", motion=None,
                     granularity=None, prog=None) -> "MadsStepper":
        """mac_mads_begin: the native loop one poll at a time over the candidate shard
        ``shard`` = (lo, hi) of each poll's 2 n_p candidates (None: the whole poll). ``cons``: as
        mads_run's (mac_mads_begin_cons; every rank of a sharded loop passes the same one).
        ``poll_vars``: as mads_run's (n_p = 3N for "xyr", 2N for "xy": mac_mads_begin_opts).
        ``motion``: as mads_run's (mac_mads_begin_motion; the same on every rank).
        ``granularity``: as mads_run's (mac_mads_begin_mesh; the same on every rank).
        ``prog``: refused (ValueError): this stepper exchanges a 16-byte best, which the progressive
        barrier cannot be decided from; use mads_prog_stepper (or mads_run)."""
        if prog is not None:
            raise ValueError("mads_stepper: prog (progressive constraints) is not supported by this "
                             "stepper; use mads_prog_stepper(prog=) or mads_run(prog=)")
        st = MadsStepper(self, x0, r_max, penalty, prev, d_lim, tan_half_fov, n_iter, ell0,
                         ell_max, seed, shard, cons, poll_vars, motion, granularity)
        self._steppers.add(st)
        return st

    def mads_prog_stepper(self, x0, r_max, penalty: float = 1e5, prev=None, d_lim=None,
                          tan_half_fov: float = 1.0, n_iter: int = 100, ell0: int = 2,
                          ell_max: int = 6, seed: int = 20250216, shard=None,
                          cons=None, poll_vars: str = "xyr", motion=None,
                          granularity=None, prog=None, h_max0=None) -> "MadsProgStepper":
        """mac_mads_begin_prog: mads_run(prog=)'s loop one iteration at a time over the candidate shard
        ``shard`` = (lo, hi) of every centre's poll (None: the whole poll), for dist.mads_prog_loop and
        dist.mads_prog_loop_speculative. The other keywords: as mads_stepper's and mads_run's; every
        rank passes the same ones. ``prog`` must hold a constraint (n_cons > 0)."""
        st = MadsProgStepper(self, x0, r_max, penalty, prev, d_lim, tan_half_fov, n_iter, ell0,
                             ell_max, seed, shard, cons, poll_vars, motion, granularity, prog, h_max0)
        self._steppers.add(st)
        return st

    # -- device-resident, stream-ordered
    def area_batch_dev(self, d_cands, three_n: int, K: int, d_area, stream=None) -> None:
        _check(self._L.mac_area_batch_dev_f64(self._h, _devptr(d_cands), int(three_n), int(K),
                                              _devptr(d_area), _stream(stream, self.device)))

    def poll_best_dev(self, d_cands, three_n: int, K: int, d_rmax, d_best, penalty: float = 1e5,
                      d_prev=None, d_dlim=None, tan_half_fov: float = 1.0, idx_base: int = 0,
                      d_obj=None, stream=None, cons=None) -> None:
        """mac_poll_best_dev_f64; with ``cons`` (a Cons, or anything make_cons takes) the masked poll
        mac_poll_best_cons_dev_f64 (stream-ordered as well; best_fetch(d_best) reads its result)."""
        args = (self._h, _devptr(d_cands), int(three_n), int(K), _devptr(d_rmax), float(penalty),
                _devptr(d_prev), _devptr(d_dlim), float(tan_half_fov), int(idx_base),
                _devptr(d_obj), _devptr(d_best), _stream(stream, self.device))
        if cons is None:
            _check(self._L.mac_poll_best_dev_f64(*args))
        else:
            cs = make_cons(cons)
            _check(self._L.mac_poll_best_cons_dev_f64(*args, ctypes.byref(cs)))

    def poll_step(self, d_cands, three_n: int, K: int, d_rmax, d_best, penalty: float = 1e5,
                  d_prev=None, d_dlim=None, tan_half_fov: float = 1.0, idx_base: int = 0,
                  d_obj=None, stream=None, fetch: bool = True):
        """A bound device poll: returns a zero-argument callable that enqueues the poll
        (mac_poll_best_dev_f64) and returns its (objective, index) (mac_best_fetch). The ctypes
        arguments are built once, so a step costs two foreign calls and nothing else on the
        host — the next poll of a MADS loop cannot start before this one's result is known."""
        h = _vp(self._h.value if isinstance(self._h, _vp) else self._h)
        poll_args = (h, _vp(_devptr(d_cands)), _i64(int(three_n)), _i64(int(K)),
                     _vp(_devptr(d_rmax)), ctypes.c_double(float(penalty)),
                     _vp(_devptr(d_prev)), _vp(_devptr(d_dlim)),
                     ctypes.c_double(float(tan_half_fov)), _i64(int(idx_base)),
                     _vp(_devptr(d_obj)), _vp(_devptr(d_best)), _vp(_stream(stream, self.device)))
        bo, bi = ctypes.c_double(), ctypes.c_int64()
        fetch_args = (h, _vp(_devptr(d_best)), _vp(_stream(stream, self.device)), ctypes.byref(bo),
                      ctypes.byref(bi))
        poll, fetch_f = self._L.mac_poll_best_dev_f64, self._L.mac_best_fetch

        def step():
            rc = poll(*poll_args)
            if rc != MAC_OK:
                _check(rc)
            rc = fetch_f(*fetch_args)
            if rc != MAC_OK:
                _check(rc)
            return bo.value, bi.value

        def enqueue():
            rc = poll(*poll_args)
            if rc != MAC_OK:
                _check(rc)

        return step if fetch else enqueue

    def poll_arm(self, d_cands, three_n: int, K: int, d_rmax, d_best, penalty: float = 1e5,
                 d_prev=None, d_dlim=None, tan_half_fov: float = 1.0, idx_base: int = 0,
                 d_obj=None, stream=None) -> int:
        """mac_poll_arm_dev_f64: the device poll enqueued behind the context's doorbell; returns
        its ticket (poll_fire releases it). See include/maxcover.h for the rules."""
        t = ctypes.c_uint64()
        _check(self._L.mac_poll_arm_dev_f64(
            self._h, _devptr(d_cands), int(three_n), int(K), _devptr(d_rmax), float(penalty),
            _devptr(d_prev), _devptr(d_dlim), float(tan_half_fov), int(idx_base),
            _devptr(d_obj), _devptr(d_best), _stream(stream, self.device), ctypes.byref(t)))
        return int(t.value)

    def poll_fire(self, ticket: int) -> None:
        _check(self._L.mac_poll_fire(self._h, int(ticket)))

    def armed_steps(self, polls, stream=None):
        """Bound armed polls for a loop of dependent polls: ``polls`` = a list of dicts of
        poll_best_dev arguments (d_cands, three_n, K, d_rmax, d_best, ...; consecutive polls on
        different d_best buffers). Returns (arm(j), fire(j), fetch(j)): arm enqueues poll j
        behind the doorbell, fire releases it, fetch returns its (objective, index) — with
        prebuilt ctypes arguments, so a loop step is fire(j), arm(j + 1) (enqueued while poll j
        runs), fetch(j)."""
        h = _vp(self._h.value if isinstance(self._h, _vp) else self._h)
        arm_f, fire_f, fetch_f = (self._L.mac_poll_arm_dev_f64, self._L.mac_poll_fire,
                                  self._L.mac_best_fetch)
        tickets = [ctypes.c_uint64() for _ in polls]
        bo, bi = ctypes.c_double(), ctypes.c_int64()
        sv = _vp(_stream(stream, self.device))
        arm_args, fetch_args = [], []
        for p, t in zip(polls, tickets):
            arm_args.append((h, _vp(_devptr(p["d_cands"])), _i64(int(p["three_n"])), _i64(int(p["K"])),
                             _vp(_devptr(p["d_rmax"])), ctypes.c_double(float(p.get("penalty", 1e5))),
                             _vp(_devptr(p.get("d_prev"))), _vp(_devptr(p.get("d_dlim"))),
                             ctypes.c_double(float(p.get("tan_half_fov", 1.0))),
                             _i64(int(p.get("idx_base", 0))), _vp(_devptr(p.get("d_obj"))),
                             _vp(_devptr(p["d_best"])), sv, ctypes.byref(t)))
            fetch_args.append((h, _vp(_devptr(p["d_best"])), sv, ctypes.byref(bo), ctypes.byref(bi)))

        def arm(j):
            rc = arm_f(*arm_args[j])
            if rc != MAC_OK:
                _check(rc)

        def fire(j):
            rc = fire_f(h, tickets[j].value)
            if rc != MAC_OK:
                _check(rc)

        def fetch(j):
            rc = fetch_f(*fetch_args[j])
            if rc != MAC_OK:
                _check(rc)
            return bo.value, bi.value

        return arm, fire, fetch

    def best_reduce_dev(self, d_records, n_records: int, d_best, stream=None) -> None:
        """mac_best_reduce_dev: the lexicographic minimum of n_records 16-B {objective, index}
        records (device) into d_best and its mapped slot, on ``stream`` (read it with best_fetch)."""
        _check(self._L.mac_best_reduce_dev(self._h, _devptr(d_records), int(n_records), _devptr(d_best),
                                           _stream(stream, self.device)))

    # -- the multi-GPU poll exchange over RCCL on the poll's stream (mac_comm_*, mac_poll_exchange)
    @staticmethod
    def comm_unique_id(rccl_path: str | None = None) -> bytes:
        """mac_comm_unique_id: a fresh 128-byte communicator id (rank 0 makes it)."""
        buf = ctypes.create_string_buffer(128)
        _check(load_library().mac_comm_unique_id(rccl_path.encode() if rccl_path else None, buf))
        return buf.raw

    def comm_init(self, uid: bytes, rank: int, world: int, rccl_path: str | None = None) -> None:
        """mac_comm_init (collective over the ranks)."""
        if len(uid) != 128:
            raise ValueError("communicator id must be 128 bytes")
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _check(self._L.mac_comm_init(self._h, rccl_path.encode() if rccl_path else None, buf,
                                     int(rank), int(world)))

    def exchange_step(self, d_best, d_out, stream=None):
        """A bound mac_poll_exchange (prebuilt ctypes arguments): returns a zero-argument callable
        giving the node's (objective, index) over every rank's 16-B d_best."""
        h = _vp(self._h.value if isinstance(self._h, _vp) else self._h)
        bo, bi = ctypes.c_double(), ctypes.c_int64()
        args = (h, _vp(_devptr(d_best)), _vp(_devptr(d_out)), _vp(_stream(stream, self.device)),
                ctypes.byref(bo), ctypes.byref(bi))
        f = self._L.mac_poll_exchange

        def step():
            rc = f(*args)
            if rc != MAC_OK:
                _check(rc)
            return bo.value, bi.value

        return step

    def exchange_records(self, rec: np.ndarray, out: np.ndarray, stream=None) -> None:
        """mac_exchange_records: rec (this rank's record, a contiguous array of 8-B words) gathered
        from every rank into out (world rows of the same size)."""
        _check(self._L.mac_exchange_records(self._h, rec.ctypes.data, int(rec.nbytes), out.ctypes.data,
                                            _stream(stream, self.device)))

    def reduce_step(self, d_records, n_records: int, d_best, stream=None):
        """A bound mac_best_reduce_dev + mac_best_fetch (prebuilt ctypes arguments): returns a
        zero-argument callable giving the reduced (objective, index)."""
        h = _vp(self._h.value if isinstance(self._h, _vp) else self._h)
        sv = _vp(_stream(stream, self.device))
        red_args = (h, _vp(_devptr(d_records)), _i32(int(n_records)), _vp(_devptr(d_best)), sv)
        bo, bi = ctypes.c_double(), ctypes.c_int64()
        fetch_args = (h, _vp(_devptr(d_best)), sv, ctypes.byref(bo), ctypes.byref(bi))
        red, fetch = self._L.mac_best_reduce_dev, self._L.mac_best_fetch

        def step():
            rc = red(*red_args)
            if rc != MAC_OK:
                _check(rc)
            rc = fetch(*fetch_args)
            if rc != MAC_OK:
                _check(rc)
            return bo.value, bi.value

        return step

    def best_fetch(self, d_best, stream=None):
        """The (objective, index) the latest device poll on d_best wrote (mac_best_fetch).
        Thread-safe: the output words are per call.

        Returns as soon as the poll's mapped result slot lands, while the poll's finalize launch
        may still be retiring: d_best itself is then valid for device work on any stream, but
        later host reads of d_obj / d_area, and reuse of the poll's inputs (candidates, d_prev,
        d_rmax), must be ordered on ``stream`` or follow a synchronisation of it."""
        bo, bi = ctypes.c_double(), ctypes.c_int64()
        _check(self._L.mac_best_fetch(self._h, _devptr(d_best), _stream(stream, self.device),
                                      ctypes.byref(bo), ctypes.byref(bi)))
        return bo.value, bi.value


class MadsStepper:
    """mac_mads_begin / _poll / _update / _result (include/maxcover.h): poll() -> (done,
    best_obj, best_idx) over this stepper's shard; update(obj, idx) with the best over all
    shards; result() -> (x, stats). dist.mads_loop drives it. ``n_polled`` is n_p (3N, or 2N under
    poll_vars="xy") and ``candidates`` = 2 n_p, every poll's candidate count; the default shard is
    (0, candidates)."""

    def __init__(self, ctx: Context, x0, r_max, penalty, prev, d_lim, tan_half_fov, n_iter,
                 ell0, ell_max, seed, shard, cons=None, poll_vars: str = "xyr", motion=None,
                 granularity=None):
        pvars = poll_vars_code(poll_vars)
        x = _f64(x0)
        g = mesh_granularity(granularity, x.size)   # (validated before the library is touched)
        self._L = ctx._L
        self._ctx = ctx   # keeps the context alive while the stepper lives
        rm = _f64(r_max)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        self.n = x.size
        self.poll_vars = poll_vars
        self.n_polled = x.size if pvars == MAC_POLL_XYR else 2 * (x.size // 3)
        self.candidates = 2 * self.n_polled
        lo, hi = (0, self.candidates) if shard is None else (int(shard[0]), int(shard[1]))
        self.shard = (lo, hi)
        prm = MadsParams(int(n_iter), int(ell0), int(ell_max), int(seed) & (2**64 - 1))
        h = _vp()
        args = (ctx._h, _ptr(x), x.size, _ptr(rm), float(penalty),
                _ptr(pv) if pv is not None else None, _ptr(dl) if dl is not None else None,
                float(tan_half_fov), ctypes.byref(prm), lo, hi, ctypes.byref(h))
        cs = make_cons(cons)
        if g is not None:   # (the library copies the vector during the call)
            op, mo = MadsOpts(pvars), make_motion(motion) if motion is not None else None
            mesh = MadsMesh(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0)
            _check(self._L.mac_mads_begin_mesh(*args, _opt(cs), ctypes.byref(op), _opt(mo),
                                               ctypes.byref(mesh)))
        elif motion is not None:
            op, mo = MadsOpts(pvars), make_motion(motion)
            _check(self._L.mac_mads_begin_motion(*args, _opt(cs), ctypes.byref(op), _opt(mo)))
        elif pvars != MAC_POLL_XYR:
            op = MadsOpts(pvars)
            _check(self._L.mac_mads_begin_opts(*args, ctypes.byref(cs) if cs is not None else None,
                                               ctypes.byref(op)))
        elif cs is None:
            _check(self._L.mac_mads_begin(*args))
        else:
            _check(self._L.mac_mads_begin_cons(*args, ctypes.byref(cs)))
        self._h = h
        self._done, self._bo, self._bi = _i32(), ctypes.c_double(), _i64()

    def poll(self):
        _check(self._L.mac_mads_poll(self._h, ctypes.byref(self._done), ctypes.byref(self._bo),
                                     ctypes.byref(self._bi)))
        return bool(self._done.value), self._bo.value, int(self._bi.value)

    def update(self, best_obj: float, best_idx: int) -> None:
        _check(self._L.mac_mads_update(self._h, float(best_obj), int(best_idx)))

    def poll_ahead(self, ahead: int):
        """mac_mads_poll_ahead: (done, best_obj, best_idx, feasible) of the poll that follows
        `ahead` failures of the current iteration, the stepper unchanged; feasible = its
        candidates that passed cons3 (and the stepper's swarm constraints)."""
        fe = _i64()
        _check(self._L.mac_mads_poll_ahead(self._h, int(ahead), ctypes.byref(self._done),
                                           ctypes.byref(self._bo), ctypes.byref(self._bi),
                                           ctypes.byref(fe)))
        return bool(self._done.value), self._bo.value, int(self._bi.value), int(fe.value)

    def advance(self, best_obj: float, best_idx: int) -> bool:
        """mac_mads_advance: apply one iteration's result; True when the incumbent moved."""
        mv = _i32()
        _check(self._L.mac_mads_advance(self._h, float(best_obj), int(best_idx), ctypes.byref(mv)))
        return bool(mv.value)

    def best_buffer(self, d_best16) -> None:
        """Later polls also write their 16-B shard best into ``d_best16`` (a device tensor of
        2 float64, or None to stop): mac_mads_best_buffer."""
        self._best_buf = d_best16   # kept alive while the stepper writes it
        _check(self._L.mac_mads_best_buffer(self._h, _devptr(d_best16) if d_best16 is not None
                                            else None))

    def result(self):
        out = np.empty(self.n)
        st = MadsStats()
        _check(self._L.mac_mads_result(self._h, _ptr(out), ctypes.byref(st)))
        return out, {k: getattr(st, k) for k, _ in MadsStats._fields_}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.mac_mads_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MadsProgStepper:
    """mac_mads_begin_prog / _poll_prog / _advance_prog / _result_prog (include/maxcover.h): poll(ahead)
    -> (done, ProgPart) over this stepper's shard of the iteration ``ahead`` chaining iterations on;
    advance(part) with the record merged over all shards -> (outcome, chains); result() -> (x, stats)
    with mads_run(prog=)'s keys. dist.mads_prog_loop and dist.mads_prog_loop_speculative drive it."""

    OUTCOMES = ("dominating", "improving", "unsuccessful")

    def __init__(self, ctx: Context, x0, r_max, penalty, prev, d_lim, tan_half_fov, n_iter,
                 ell0, ell_max, seed, shard, cons=None, poll_vars: str = "xyr", motion=None,
                 granularity=None, prog=None, h_max0=None):
        pvars = poll_vars_code(poll_vars)
        x = _f64(x0)
        g = mesh_granularity(granularity, x.size)   # (validated before the library is touched)
        pg = make_prog(prog, h_max0=h_max0)
        if pg is None or pg.n_cons <= 0:
            raise ValueError("mads_prog_stepper: prog must hold a progressive constraint (use mads_stepper)")
        if pg.n_uav != x.size // 3:
            raise ValueError("prog: member and limit hold N values each")
        self._L = ctx._L
        self._ctx = ctx   # keeps the context alive while the stepper lives
        rm = _f64(r_max)
        pv = _f64(prev) if prev is not None else None
        dl = _f64(d_lim) if d_lim is not None else None
        self.n = x.size
        self.poll_vars = poll_vars
        self.n_polled = x.size if pvars == MAC_POLL_XYR else 2 * (x.size // 3)
        self.candidates = 2 * self.n_polled
        lo, hi = (0, self.candidates) if shard is None else (int(shard[0]), int(shard[1]))
        self.shard = (lo, hi)
        prm = MadsParams(int(n_iter), int(ell0), int(ell_max), int(seed) & (2**64 - 1))
        h = _vp()
        op, mo = MadsOpts(pvars), make_motion(motion) if motion is not None else None
        mesh = MadsMesh(g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0) if g is not None else None
        cs = make_cons(cons)
        _check(self._L.mac_mads_begin_prog(
            ctx._h, _ptr(x), x.size, _ptr(rm), float(penalty), _ptr(pv) if pv is not None else None,
            _ptr(dl) if dl is not None else None, float(tan_half_fov), ctypes.byref(prm), lo, hi,
            ctypes.byref(h), _opt(cs), ctypes.byref(op), _opt(mo), _opt(mesh), ctypes.byref(pg)))
        self._h = h
        self._done = _i32()

    def poll(self, ahead: int = 0):
        part = ProgPart()
        _check(self._L.mac_mads_poll_prog(self._h, int(ahead), ctypes.byref(self._done), ctypes.byref(part)))
        return bool(self._done.value), part

    def advance(self, part):
        """mac_mads_advance_prog: (outcome, chains): 'dominating' / 'improving' / 'unsuccessful', and
        whether a record polled one iteration ahead applies next."""
        if not isinstance(part, ProgPart):
            part = ProgPart.from_words(part)
        oc, ch = _i32(), _i32()
        _check(self._L.mac_mads_advance_prog(self._h, ctypes.byref(part), ctypes.byref(oc), ctypes.byref(ch)))
        return self.OUTCOMES[oc.value], bool(ch.value)

    def result(self):
        out = np.empty(self.n)
        xi = np.full(self.n, np.nan)
        st, ps = MadsStats(), MadsProgStats()
        _check(self._L.mac_mads_result_prog(self._h, _ptr(out), _ptr(xi), ctypes.byref(st), ctypes.byref(ps)))
        stats = {k: getattr(st, k) for k, _ in MadsStats._fields_}
        stats.update({k: getattr(ps, k) for k, _ in MadsProgStats._fields_})
        stats["x_infeasible"] = xi if ps.has_infeasible else None
        return out, stats

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.mac_mads_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fcheck(rc: int) -> None:
    if rc != MAC_OK:
        raise MaxCoverError(rc, load_library().mac_fire_last_error().decode(errors="replace"))


class Fire:
    """The GPU cellular-automaton fire of src/DynamicArea.jl (mac_fire_*, include/maxcover.h).

    ``ignition`` = (ix0, ix1, iy0, iy1): 1-based inclusive cell block set on fire (:35)."""

    def __init__(self, nx: int, ny: int, dx: float, dy: float, forest_density: float,
                 prob_spread: float, wind_speed: float, wind_direction: float, ignition,
                 seed: int, device: int = 0):
        L = load_library()
        self._L = L
        ix0, ix1, iy0, iy1 = (int(v) for v in ignition)
        self.params = FireParams(int(nx), int(ny), float(dx), float(dy), float(forest_density),
                                 float(prob_spread), float(wind_speed), float(wind_direction),
                                 ix0, ix1, iy0, iy1, int(seed) & (2**64 - 1))
        h = _vp()
        _fcheck(L.mac_fire_create(ctypes.byref(h), int(device), ctypes.byref(self.params)))
        self._h = h
        self.nx, self.ny = int(nx), int(ny)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._L.mac_fire_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def thresholds(self) -> np.ndarray:
        out = np.zeros(9)
        self._L.mac_fire_thresholds(ctypes.byref(self.params), _ptr(out))
        return out

    def initial_points(self) -> np.ndarray:
        n = _i64()
        _fcheck(self._L.mac_fire_initial_points(self._h, None, 0, ctypes.byref(n)))
        rec = np.zeros((max(n.value, 1), 5))
        _fcheck(self._L.mac_fire_initial_points(self._h, _ptr(rec), n.value, ctypes.byref(n)))
        return rec[: n.value]

    def step(self, append_to: Context | None = None) -> int:
        """One update_grid step (:52-72); the new points are appended to ``append_to``'s list
        (update_POI) when given. Returns how many points were pushed."""
        n = _i64()
        ctx = append_to._h if append_to is not None else None
        _fcheck(self._L.mac_fire_step(self._h, ctx, ctypes.byref(n)))
        return int(n.value)

    def last_points(self) -> np.ndarray:
        """The last step's points as (n, 5) records, in the reference's push order."""
        n = _i64()
        _fcheck(self._L.mac_fire_last_points(self._h, None, 0, ctypes.byref(n)))
        rec = np.zeros((max(n.value, 1), 5))
        _fcheck(self._L.mac_fire_last_points(self._h, _ptr(rec), n.value, ctypes.byref(n)))
        return rec[: n.value]

    def grid(self) -> np.ndarray:
        g = np.empty(self.nx * self.ny, dtype=np.uint8)
        _fcheck(self._L.mac_fire_get_grid(self._h, g.ctypes.data_as(_u8p)))
        return g.reshape(self.nx, self.ny)

    def set_grid(self, g) -> None:
        g = np.ascontiguousarray(np.asarray(g, dtype=np.uint8).reshape(-1))
        if g.size != self.nx * self.ny:
            raise ValueError("grid size mismatch")
        _fcheck(self._L.mac_fire_set_grid(self._h, g.ctypes.data_as(_u8p)))


_default_ctx = None
_default_lock = threading.Lock()


def default_context() -> Context:
    """Process-wide context on LOCAL_RANK's GPU (device 0 by default)."""
    global _default_ctx
    with _default_lock:
        if _default_ctx is None:
            _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
        return _default_ctx
