"""Mirror of the extreme constraints the driver passes to MADS (src/TDM_Constraints.jl):
``cons1`` (:9-19, always true) and ``create_cons3`` (:54-75, per-UAV 3-D displacement limit).
The returned ``cons3`` evaluates on the host with the reference's arithmetic and also carries
its data (``prev``, ``d_lim``, ``tan_half_fov``) so the batched GPU poll can apply the same
test inside libmaxcover (finalize kernel, exact threshold form).

``create_cons8`` (:157-172, minimum spacing) and ``create_cons7`` (:142-154, altitude zone) are the
swarm constraints written for the reference's ``cons_ext`` slot; they carry ``mac_cons`` fields, which
``TDM_STATIC_opt.mads`` merges into one descriptor for the device (include/maxcover.h mac_cons)."""
from __future__ import annotations

import math

import numpy as np


def cons1(x) -> bool:
    """src/TDM_Constraints.jl:9-19 — the body is commented out; always feasible."""
    return True


def create_cons3(pre_optimized_circles_MADS, FOV: float, d_lim):
    """src/TDM_Constraints.jl:54-75. ``pre_optimized_circles_MADS``: list of Circle or [x;y;R]."""
    from .AreaCoverageCalculation import make_MADS
    pre = pre_optimized_circles_MADS
    if len(pre) and not isinstance(pre[0], (float, int, np.floating, np.integer)):
        prev = make_MADS(pre)
    else:
        prev = np.asarray(pre, dtype=np.float64)
    prev = np.ascontiguousarray(prev, dtype=np.float64)
    dl = np.ascontiguousarray(np.asarray(d_lim, dtype=np.float64))
    t = math.tan(FOV / 2)

    def cons3(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            x1, y1, z1 = float(prev[i]), float(prev[N + i]), float(prev[2 * N + i]) / t
            x2, y2, z2 = float(xx[i]), float(xx[N + i]), float(xx[2 * N + i]) / t
            if math.sqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2)) \
                    > dl[i]:
                return False
        return True

    cons3.prev = prev
    cons3.d_lim = dl
    cons3.tan_half_fov = t
    return cons3


def create_cons7(FOV: float, y_below: float = 200.0, h_above: float = 19.0):
    """src/TDM_Constraints.jl:142-154 (altitude cap inside a zone): infeasible when a UAV with
    y < y_below has R > h_above * tan(FOV/2). The reference reads N, FOV and the two numbers from
    its globals; here they are arguments. Carries ``mac_cons`` (zone_y, zone_r) for the device."""
    y_lim = float(y_below)
    r_lim = float(h_above) * math.tan(FOV / 2)

    def cons7(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            if float(xx[i + N]) < y_lim:
                if float(xx[i + 2 * N]) > r_lim:
                    return False
        return True

    cons7.mac_cons = {"zone_y": y_lim, "zone_r": r_lim}
    return cons7


def create_cons8(d_sep: float = 15.0):
    """src/TDM_Constraints.jl:157-172 (minimum horizontal spacing between any two UAVs), 15.0 in
    the reference. Carries ``mac_cons`` (d_sep) for the device."""
    d = float(d_sep)

    def cons8(x) -> bool:
        xx = np.asarray(x, dtype=np.float64)
        N = xx.size // 3
        for i in range(N):
            for j in range(N):
                if j != i:
                    dx = float(xx[i]) - float(xx[j])
                    dy = float(xx[i + N]) - float(xx[j + N])
                    hor_separation = math.sqrt(dx * dx + dy * dy)
                    if hor_separation < d:
                        return False
        return True

    cons8.mac_cons = {"d_sep": d}
    return cons8


def merge_mac_cons(constraints):
    """One mac_cons dict {d_sep, zone_y, zone_r} out of the callables that carry ``mac_cons`` data
    (None when there is none), and the list of the callables that do not. Two constraints of one
    kind cannot share the descriptor's single slot: the later one stays a host callable."""
    merged, plain = {}, []
    for c in constraints:
        data = getattr(c, "mac_cons", None)
        if data and not (set(data) & set(merged)):
            merged.update(data)
        else:
            plain.append(c)
    return (merged or None), plain
