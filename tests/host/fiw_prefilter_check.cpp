// Host check of the fused chain's neighbour prefilter (csrc/fiw_box.h): for random and adversarial
// disks, grids and displacement bounds,
//     box_pre_rejects(...)  =>  !(sup_box_tiles(...) non-empty and overlapping box i),
// i.e. the prefilter only ever passes a superset of what the full test passes. Prints the counts and
// exits 0, or prints the first counterexamples and exits 1. Built and run by
// tests/test_fiw_prefilter_host.py (g++ -ffp-contract=off; no GPU).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "fiw_box.h"

namespace {

struct Rng {   // SplitMix64
    uint64_t s;
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double range(double a, double b) { return a + (b - a) * uni(); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct GridH {
    double gx0, gy0, S, invS;
    int nTx, nTy;
};

bool overlap(const int* a, const int* b)   // k_common.h box_overlap
{
    return a[0] <= a[1] && a[0] <= b[1] && b[0] <= a[1] && a[2] <= b[3] && b[2] <= a[3];
}

long g_tested = 0, g_rejected = 0, g_full_rejected = 0, g_bad = 0, g_boxes = 0, g_far = 0, g_far_kept = 0;

// disk i's box under the bound D = (dx, dy, dr), then every disk of js against it
void check(const GridH& g, const double* di, const double* D, const std::vector<double>& js)
{
    int bi[4];
    if (!mac::sup_box_tiles(di[0], di[1], di[2], D[0], D[1], D[2], g.gx0, g.gy0, g.invS, g.nTx, g.nTy, bi[0],
                            bi[1], bi[2], bi[3]))
        return;   // (the kernel tests no neighbour for an empty box)
    ++g_boxes;
    const mac::BoxPre bp = mac::box_pre(bi[0], bi[1], bi[2], bi[3], D[0], D[1], g.gx0, g.gy0, g.S, g.invS);
    for (size_t q = 0; q + 2 < js.size(); q += 3) {
        const double x0 = js[q], y0 = js[q + 1], r0 = js[q + 2];
        int bj[4] = {0, -1, 0, -1};
        const bool full = mac::sup_box_tiles(x0, y0, r0, D[0], D[1], D[2], g.gx0, g.gy0, g.invS, g.nTx, g.nTy,
                                             bj[0], bj[1], bj[2], bj[3]) &&
                          overlap(bj, bi);
        const bool rej = mac::box_pre_rejects(bp, x0, y0, r0 + D[2]);
        ++g_tested;
        g_rejected += rej;
        g_full_rejected += !full;
        // (and it is no empty promise: a disk plainly out of reach — beyond the bound's T by a
        // thousandth, at magnitudes where the relative slack is smaller than that — is rejected)
        const double T = r0 + D[2] + bp.c;
        const double M = std::fabs(x0) + std::fabs(y0) + T + bp.m;
        if (T > 0.0 && M <= 1e150 && M * 1e-9 < 1e-3 * T &&
            (std::fabs(x0 - bp.cx) > 1.002 * T || std::fabs(y0 - bp.cy) > 1.002 * T)) {
            ++g_far;
            g_far_kept += !rej;
        }
        if (rej && full) {
            if (g_bad++ < 10)
                std::printf("COUNTEREXAMPLE grid (%a %a S %a n %d %d) i (%a %a %a) D (%a %a %a) j (%a %a %a)\n",
                            g.gx0, g.gy0, g.S, g.nTx, g.nTy, di[0], di[1], di[2], D[0], D[1], D[2], x0, y0, r0);
        }
    }
}

double nudge(double v, int ulps)
{
    for (int q = 0; q < std::abs(ulps); ++q) v = std::nextafter(v, ulps > 0 ? INFINITY : -INFINITY);
    return v;
}

}  // namespace

int main()
{
    Rng rng{20250216};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double pitches[] = {1.0, 5.0, 0.37, 1e-3, 1e3, 64.0, 1e-9, 3e7};
    const double specials[] = {0.0, -0.0, 1.0, -1.0, 1e-300, 1e150, 1e155, 1e300, -1e300, 1.7e308, inf, -inf, nan,
                               4503599627370496.0, 1e16, -1e16};
    const int nspecial = (int)(sizeof(specials) / sizeof(specials[0]));
    for (int trial = 0; trial < 4000; ++trial) {
        GridH g;
        g.S = pitches[rng.below(8)];
        g.invS = 1.0 / g.S;
        g.nTx = 1 + rng.below(trial % 7 == 0 ? 3 : 400);
        g.nTy = 1 + rng.below(trial % 11 == 0 ? 3 : 400);
        const double off = trial % 5 == 0 ? rng.range(-1e9, 1e9) * g.S : rng.range(-100.0, 100.0) * g.S;
        g.gx0 = off;
        g.gy0 = trial % 3 == 0 ? -off : rng.range(-50.0, 50.0) * g.S;
        const double W = g.nTx * g.S, H = g.nTy * g.S;
        // the displacement bound: integers (a MADS mesh), fractions, zero, huge, negative dr
        double D[3] = {std::floor(rng.range(0.0, 9.0)), std::floor(rng.range(0.0, 9.0)), std::floor(rng.range(-3.0, 9.0))};
        if (trial % 4 == 1) { D[0] = rng.range(0.0, 3.0) * g.S; D[1] = rng.range(0.0, 3.0) * g.S; D[2] = rng.range(-1.0, 2.0) * g.S; }
        if (trial % 50 == 7) D[rng.below(3)] = specials[rng.below(nspecial)];
        // disk i: inside the grid, on its edge, or outside it
        double di[3] = {g.gx0 + rng.range(-0.2, 1.2) * W, g.gy0 + rng.range(-0.2, 1.2) * H,
                        rng.range(0.1, 12.0) * g.S};
        if (trial % 9 == 0) di[2] = rng.range(0.5, 2.0) * (W + H);
        if (trial % 60 == 13) di[rng.below(3)] = specials[rng.below(nspecial)];
        int bi[4];
        const bool any = mac::sup_box_tiles(di[0], di[1], di[2], D[0], D[1], D[2], g.gx0, g.gy0, g.invS, g.nTx,
                                            g.nTy, bi[0], bi[1], bi[2], bi[3]);
        std::vector<double> js;
        auto put = [&](double x, double y, double r) { js.push_back(x); js.push_back(y); js.push_back(r); };
        for (int q = 0; q < 40; ++q)   // anywhere
            put(g.gx0 + rng.range(-1.0, 2.0) * W, g.gy0 + rng.range(-1.0, 2.0) * H, rng.range(-1.0, 14.0) * g.S);
        if (any) {
            // tile edges: disk j's reach x0 -+ (dx + R) on, and a few ulps and tiles around, every
            // edge of box i's tiles, on each axis, the other axis inside or at a corner
            for (int side = 0; side < 2; ++side)
                for (int axis = 0; axis < 2; ++axis)
                    for (int dt = -2; dt <= 2; ++dt)
                        for (int ul = -3; ul <= 3; ++ul) {
                            const double r = rng.range(0.2, 6.0) * g.S, R = r + D[2];
                            const double reach = D[axis] + R;
                            const double g0 = axis ? g.gy0 : g.gx0;
                            const int t = side ? bi[2 * axis + 1] + 1 + dt : bi[2 * axis] + dt;
                            const double edge = g0 + (double)t * g.S;
                            const double c = nudge(side ? edge + reach : edge - reach, ul * (1 + 5 * (ul & 1)));
                            const int oa = 1 - axis;
                            const double og0 = oa ? g.gy0 : g.gx0;
                            double o = og0 + 0.5 * (double)(bi[2 * oa] + bi[2 * oa + 1] + 1) * g.S;
                            if (dt & 1) o = og0 + (double)(bi[2 * oa + 1] + 1) * g.S + D[oa] + R;   // a corner
                            if (axis) put(o, c, r); else put(c, o, r);
                        }
        }
        for (int q = 0; q < 24; ++q) {   // huge, tiny, non-finite and negative values in every place
            double v[3] = {g.gx0 + rng.range(-1.0, 2.0) * W, g.gy0 + rng.range(-1.0, 2.0) * H, rng.range(0.1, 9.0) * g.S};
            v[rng.below(3)] = specials[rng.below(nspecial)];
            if (q % 4 == 0) v[rng.below(3)] = specials[rng.below(nspecial)];
            if (q % 6 == 0) v[2] = -rng.range(0.0, 20.0);
            put(v[0], v[1], v[2]);
        }
        check(g, di, D, js);
    }
    std::printf("boxes %ld tests %ld prefilter-rejected %ld full-test-rejected %ld far %ld far-kept %ld "
                "counterexamples %ld\n",
                g_boxes, g_tested, g_rejected, g_full_rejected, g_far, g_far_kept, g_bad);
    if (g_bad || g_boxes < 1000 || g_far < 10000 || g_far_kept) return 1;
    return 0;
}
