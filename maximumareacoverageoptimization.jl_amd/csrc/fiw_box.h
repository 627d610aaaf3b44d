// fiw_box.h — the fused chain's superset boxes (k_fiw.h) and the prefilter of its neighbour test,
// shared by host and device code (tests/host/fiw_prefilter_check.cpp runs them on the CPU).
#pragma once

#include "predicate.h"

#pragma clang fp contract(off)

namespace mac {

// Tile range [lo, hi] holding the span (predicate.h tile_span) of every disk (c, r) with
// a <= c - r, c + r <= b and |c| + r <= m: partial_range's steps (k_prep.h) with a margin 100x
// wider, which dominates every rounding by which a, b and m — computed from a base disk and the
// displacement bound — can differ from the values tile_span rounds per disk.
MAC_HD bool sup_range(double a, double b, double m, double g0, double invS, int n, int& lo, int& hi)
{
    const double ulo = (a - g0) * invS;
    const double uhi = (b - g0) * invS;
    const double err = (m + __builtin_fabs(g0)) * invS * 1e-12 + 1e-9;
    const double flo = __builtin_floor(ulo - err);
    const double fhi = __builtin_floor(uhi + err);
    if (!(flo == flo) || !(fhi == fhi)) { lo = 0; hi = n - 1; return true; }
    if (fhi < 0.0 || flo > (double)(n - 1)) return false;
    lo = flo < 0.0 ? 0 : (int)flo;
    hi = fhi > (double)(n - 1) ? n - 1 : (int)fhi;
    return true;
}

// The superset box [a0, a1] x [b0, b1] of disk (x0, y0, r0) (candidate 0's) under the displacement
// bound (dx, dy, dr): it holds the tile span of every live candidate's disk of that UAV. False:
// empty (no live disk covers anything); NaN anywhere: the whole grid.
MAC_HD bool sup_box_tiles(double x0, double y0, double r0, double dx, double dy, double dr, double gx0,
                          double gy0, double invS, int nTx, int nTy, int& a0, int& a1, int& b0, int& b1)
{
    const double R = r0 + dr;
    if (!(R > 0.0) && R == R) return false;
    if (!sup_range(x0 - dx - R, x0 + dx + R, __builtin_fabs(x0) + dx + R, gx0, invS, nTx, a0, a1))
        return false;
    if (!sup_range(y0 - dy - R, y0 + dy + R, __builtin_fabs(y0) + dy + R, gy0, invS, nTy, b0, b1))
        return false;
    return true;
}

// Prefilter of "sup_box_tiles(x0, y0, r0, dx, dy, dr) is non-empty and overlaps the box
// [a0, a1] x [b0, b1]" (a box inside the grid: disk i's own): a dozen fp64 operations in place of
// sup_box_tiles' sixty. It may only reject what the full test rejects.
//
// Per axis the full test passes only if floor(ulo - err) <= a1 and floor(uhi + err) >= a0 (the clamp
// to the grid changes neither, [a0, a1] lying inside it), with ulo = ((x0 - dx - R) - g0) invS,
// uhi = ((x0 + dx + R) - g0) invS and err = (|x0| + dx + R + |g0|) invS 1e-12 + 1e-9. In
// coordinates, with c = g0 + (a0 + a1 + 1) S / 2 the centre and h = (a1 - a0 + 1) S / 2 the half
// width of the box's tiles, passing needs
//     |x0 - c| < dx + R + h + S err + e,
// e the roundings: each of sup_range's four operations before the floor and each of the ones
// below is off by at most 2^-53 of a magnitude below M = |x0| + |y0| + |c| + h + dx + dy + R + |g0|
// (or M invS, in tiles), and S invS differs from 1 by at most 2^-52, so e < 20 x 2^-52 M and
// S err + e < 1.01e-12 M + 1e-9 S. The prefilter rejects only when
//     |x0 - c| > T + 1e-9 (|x0| + |y0| + T + m),   T = R + max(dx + hx, dy + hy) + 2 S,
//     m = |gx0| + |gy0| + |cx| + |cy|,
// (or the same with y0, cy) whose right side exceeds dx + R + h by 2 S + 1e-9 M' with M' >= M / 2:
// five hundred times S err + e. It never rejects when a value is NaN (the comparison is false), when
// the magnitudes pass 1e150 or the bound is not plainly finite and >= 0 (sup_range's own NaN rule, the
// whole grid, needs an overflow), and R <= 0 is sup_box_tiles' own "empty".
struct BoxPre {
    double cx, cy, c, m;   // c: max(dx + hx, dy + hy) + 2 S, NaN: the prefilter is off
};

MAC_HD BoxPre box_pre(int a0, int a1, int b0, int b1, double dx, double dy, double gx0, double gy0, double S,
                      double invS)
{
    BoxPre p;
    const double hx = 0.5 * (double)(a1 - a0 + 1) * S, hy = 0.5 * (double)(b1 - b0 + 1) * S;
    p.cx = gx0 + 0.5 * (double)(a0 + a1 + 1) * S;
    p.cy = gy0 + 0.5 * (double)(b0 + b1 + 1) * S;
    const double ex = dx + hx, ey = dy + hy;
    p.c = (ex > ey ? ex : ey) + 2.0 * S;
    p.m = __builtin_fabs(gx0) + __builtin_fabs(gy0) + __builtin_fabs(p.cx) + __builtin_fabs(p.cy);
    const bool ok = a0 <= a1 && b0 <= b1 && dx >= 0.0 && dy >= 0.0 && S >= 1e-100 && S <= 1e100 &&
                    invS >= 1e-100 && invS <= 1e100 && __builtin_fabs(S * invS - 1.0) <= 1e-12 &&
                    p.c <= 1e150 && p.m <= 1e150;
    if (!ok) p.c = __builtin_nan("");
    return p;
}

// R = r0 + dr, as sup_box_tiles computes it
MAC_HD bool box_pre_rejects(const BoxPre& p, double x0, double y0, double R)
{
    const double T = R + p.c;
    const double M = __builtin_fabs(x0) + __builtin_fabs(y0) + T + p.m;
    const double lim = T + M * 1e-9;
    const bool far = __builtin_fabs(x0 - p.cx) > lim || __builtin_fabs(y0 - p.cy) > lim;
    return far && M <= 1e150;
}

}  // namespace mac
