// k_cons.h — the swarm constraints of src/TDM_Constraints.jl evaluated on the device, one
// feasibility byte per candidate (mac_cons, include/maxcover.h), and the masked poll argmin.
//
//   cons8 (:157-172)  infeasible iff some i != j has sqrt((x_i-x_j)^2 + (y_i-y_j)^2) < d_sep
//   cons7 (:142-154)  infeasible iff some i has y_i < zone_y && r_i > zone_r
//
// cons8's pair test is the coverage predicate (predicate.h): with a = fl(fl(dx*dx) + fl(dy*dy)),
// fl(sqrt a) < d  <=>  a <= T(d). dx = fl(x_i - x_j) and fl(x_j - x_i) differ in sign only (rounding
// to nearest is symmetric), so a is the same for (i, j) and (j, i) and every unordered pair is
// tested once. A UAV with a NaN or infinite x or y has a = inf or NaN against every other UAV
// (dx or dy is inf or NaN, and nothing finite cancels it), and neither satisfies a <= T for any T
// (T <= DBL_MAX): it violates with nobody and is left out of the pair tests.
//
// The cull. A pair with |fl(x_j - x_i)| >= dcut is skipped without its fp64 test. Claim: with
// dcut = d_sep every skipped pair is feasible, provided D2 := fl(d_sep * d_sep) > T(d_sep) — which the
// host checks for the d_sep at hand (cons_args below; it holds for every d_sep whose square neither
// overflows nor loses bits to the subnormal range, because sqrt(fl(d*d)) rounds back to d in binary
// floating point; it fails e.g. for d_sep = 1e-200, where D2 = 0 <= T, and the host then passes
// dcut = +inf, which only skips dx = +-inf, i.e. a = inf: feasible).
//   1. dx := fl(x_j - x_i), |dx| >= d_sep > 0 (possibly inf by overflow), so as reals
//      dx*dx >= d_sep*d_sep, and by monotone rounding fl(dx*dx) >= D2.
//   2. dy is finite or +-inf (both y finite), so fl(dy*dy) >= 0 and is not NaN; hence
//      fl(dx*dx) + fl(dy*dy) >= fl(dx*dx) as extended reals, and a = fl(of that sum) >=
//      fl(dx*dx) >= D2 (rounding is monotone and leaves the double fl(dx*dx) fixed).
//   3. a >= D2 > T  =>  not (a <= T)  =>  not (fl(sqrt a) < d_sep): the pair is feasible.
// Whole runs of pairs are skipped the same way. The finite UAVs are counting-sorted in LDS into
// kConsCells cells along x with boundaries bnd[0] = min x <= bnd[1] <= ... (doubles, non-decreasing);
// a UAV's cell g is guessed by a division and then corrected against the boundaries themselves until
// bnd[g] <= x (and x < bnd[g + 1] unless g is the last cell), so that inequality holds exactly and
// does not depend on how the guess rounded. The sorted positions are ordered by cell (in any order
// inside a cell). The UAV at position p (x_i) is tested against the positions q > p, and stops at the
// first later cell c with fl(bnd[c] - x_i) >= dcut: every position from there on has
// x_j >= bnd[its cell] >= bnd[c], subtraction rounds monotonically, so fl(x_j - x_i) >=
// fl(bnd[c] - x_i) >= dcut and the pair is feasible by 1-3. Every unordered pair of finite UAVs is
// thus either tested (from its lower position) or proven feasible. Cells are at least dcut wide, so a
// UAV meets its own cell and the next one or two; with dcut = +inf all UAVs share cell 0 and every
// pair is tested. No finite UAV is lost: each takes one slot of its cell from an atomic cursor. The
// order inside a cell depends on the atomics; the result, an OR over pairs, does not.
//
// The target-motion constraints (mac_motion, include/maxcover.h) are per UAV and per candidate. With
// the anchor a (the previous target) and t = (x_i - a.x_i, y_i - a.y_i, r_i - a.r_i),
// q2 = fl(fl(tx*tx) + fl(ty*ty)) and q3 = fl(q2 + fl(tz*tz)), a candidate is infeasible iff some i has
//   cons5 (:106-119)  fl(sqrt q3) > v_max                <=>  q3 > dlim_threshold(v_max)
//   cons6 (:122-138)  |fl(sqrt q3) - p_i| > a_max        <=>  q3 > Qhi_i || q3 <= Qlo_i
//   cons4 (:78-103)   fl(dot(u_i, t.xy) / fl(|u_i| * fl(sqrt q2))) < cone_cos
// Qhi_i / Qlo_i are built on the host (motion_thresholds below): fl(s - p) is monotone in
// s = fl(sqrt q3), so "fl(s - p) > a" holds from one double s_hi on, i.e. iff !(s < s_hi) iff
// q3 > T(s_hi); "fl(p - s) > a" holds up to one double s_lo, i.e. iff s < next_up(s_lo) iff
// q3 <= T(next_up(s_lo)). |u_i| = fl(sqrt(fl(ux*ux) + fl(uy*uy))) comes from the host as well. cons4
// alone needs a square root and a division on the device (both fp64, correctly rounded without
// fast-math); a zero velocity or a zero move gives 0/0 = NaN, which no comparison rejects. The tests
// sit in cons_violates' loader (MOT, a compile-time flag: the instantiations without it are the code
// they were); with d_sep off there is no sort at all (motion_violates).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "predicate.h"
#include "k_common.h"
#include "k_final.h"
#include "k_prep.h"

#pragma clang fp contract(off)

namespace mac {

constexpr int kConsMaxN = 2048;     // UAVs sorted in LDS: x and y, 16 B each (dynamic LDS, 32 KB)
constexpr int kConsBlock = 256;
constexpr int kConsCells = 256;     // cells of the counting sort by x (one per thread)
constexpr int kConsArgminBlock = 1024;

struct ConsArgs {
    double T;        // cover_threshold(d_sep): the pair is infeasible iff a <= T
    double dcut;     // the sweep's cut: d_sep when fl(d_sep*d_sep) > T, else +inf (see above)
    double zone_y;   // cons7
    double zone_r;
    int sep;         // cons8 on (d_sep > 0)
    int zone;        // cons7 on (neither field NaN)
};

// Elements per thread of the sort: the sorted array holds P = 256 S >= N entries (S = 1, 2, 4, 8).
static inline int cons_slots(int N)
{
    int S = 1;
    while (kConsBlock * S < N) S <<= 1;
    return S;
}

static inline ConsArgs cons_args(double d_sep, double zone_y, double zone_r)
{
    ConsArgs a;
    a.sep = d_sep > 0.0 ? 1 : 0;   // (NaN: off)
    a.T = cover_threshold(d_sep);
    const double d2 = d_sep * d_sep;
    a.dcut = (a.sep && d2 > a.T) ? d_sep : __builtin_inf();
    a.zone = (zone_y == zone_y && zone_r == zone_r) ? 1 : 0;
    a.zone_y = zone_y;
    a.zone_r = zone_r;
    return a;
}

// The motion constraints' device arguments: per-UAV arrays (one upload per call or stepper) and the
// scalars. A constraint that is off has its flag 0 and its arrays unread.
struct MotionArgs {
    const double* anchor;   // 3N: [x; y; R] of the previous target
    const double* vel;      // 2N: [vx; vy]                              (cons4)
    const double* un;       // N: fl(sqrt(fl(vx*vx) + fl(vy*vy)))         (cons4)
    const double* qhi;      // N: infeasible iff q3 > qhi[i] ...          (cons6)
    const double* qlo;      // N: ... or q3 <= qlo[i]
    double cone_cos;        // cons4: infeasible iff c < cone_cos
    double q5;              // cons5: infeasible iff q3 > q5 = dlim_threshold(v_max)
    int cone, speed, accel;
};

// Doubles s >= 0 in their order, by bit pattern: 0 .. kMotionInfBits (+inf).
constexpr uint64_t kMotionInfBits = 0x7ff0000000000000ull;

// cons6's thresholds for one UAV (p = speed_prev[i], a = a_max; a NaN in either: neither side ever
// rejects): see the header. The two
// boundaries are found by bisection over the non-negative doubles (the predicates are monotone in
// s because a correctly rounded subtraction is), so they are exact whatever p and a are.
//   qhi = T(s_hi), s_hi the smallest s in [0, +inf] with fl(s - p) > a   (+inf when there is none)
//   qlo = T(next_up(s_lo)), s_lo the largest s in [0, +inf] with fl(p - s) > a   (-1 when none)
static inline void motion_thresholds(double p, double a, double* qhi, double* qlo)
{
    auto dbl = [](uint64_t b) { return __builtin_bit_cast(double, b); };
    auto up = [&](uint64_t b) { const volatile double d = dbl(b) - p; return d > a; };
    auto dn = [&](uint64_t b) { const volatile double d = p - dbl(b); return d > a; };
    *qhi = __builtin_inf();
    *qlo = -1.0;
    if (p != p || a != a) return;   // every comparison false
    // p = +inf makes fl(s - p) NaN at s = +inf only: the search runs over the finite s and +inf is
    // looked at on its own
    if (up(0)) {
        *qhi = cover_threshold(0.0);   // -1: every q3 that is not NaN
    } else {
        uint64_t lo = 0, hi = kMotionInfBits - 1;   // up(lo) false; hi: the largest finite
        if (up(hi)) {
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (up(mid)) hi = mid; else lo = mid;
            }
            *qhi = cover_threshold(dbl(hi));
        } else if (up(kMotionInfBits)) {
            *qhi = cover_threshold(__builtin_inf());   // DBL_MAX: q3 = +inf only
        }
    }
    if (dn(0)) {
        uint64_t lo = 0, hi = kMotionInfBits;   // dn(lo) true
        if (dn(hi)) {
            lo = hi;
        } else {
            while (hi - lo > 1) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (dn(mid)) lo = mid; else hi = mid;
            }
        }
        // s <= s_lo  <=>  s < next_up(s_lo)  <=>  q3 <= T(next_up(s_lo)); s_lo = +inf: every q3
        *qlo = lo == kMotionInfBits ? __builtin_inf() : cover_threshold(next_up(dbl(lo)));
    }
}

// cons7's test of one UAV at (y, r), as the loaders of cons_violates and motion_violates spell it (they
// keep their own line: a call here compiled cons_mask_kernel to other code); cons_explain's form.
__device__ __forceinline__ bool zone_rejects(const ConsArgs& a, double y, double r)
{
    return a.zone && y < a.zone_y && r > a.zone_r;
}

// The motion tests of UAV e at (x, y, r) (r is read only under cons5 / cons6).
__device__ __forceinline__ bool motion_rejects(const MotionArgs& m, int e, int N, double x, double y, double r)
{
    const double tx = x - m.anchor[e], ty = y - m.anchor[N + e];
    const double q2 = tx * tx + ty * ty;
    bool bad = false;
    if (m.speed | m.accel) {
        const double tz = r - m.anchor[2 * N + e];
        const double q3 = q2 + tz * tz;
        bad = m.speed && q3 > m.q5;
        if (m.accel) bad |= q3 > m.qhi[e] || q3 <= m.qlo[e];
    }
    if (m.cone) {
        const double ux = m.vel[e], uy = m.vel[N + e];
        const double c = (ux * tx + uy * ty) / (m.un[e] * __builtin_sqrt(q2));
        bad |= c < m.cone_cos;
    }
    return bad;
}

// A candidate under the motion constraints (and cons7) with d_sep off: no pair test, so no sort, no
// extent reduction and no LDS arrays. A load, the tests and one flag.
template <int S, class Load>
__device__ __forceinline__ bool motion_violates(Load load, int N, const ConsArgs& a, const MotionArgs& m)
{
    bool bad = false;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = s * kConsBlock + (int)threadIdx.x;
        if (e < N) {
            double x, y, r;
            load(e, x, y, r);
            bad |= a.zone && y < a.zone_y && r > a.zone_r;
            bad |= motion_rejects(m, e, N, x, y, r);
        }
    }
    return __syncthreads_or(bad ? 1 : 0) != 0;
}

// The sort-and-sweep of one candidate by one workgroup, shared by the matrix and the generated-poll
// kernels: load(e, x, y, r) gives UAV e's values (r is read only under cons7). Thread t loads
// elements s * 256 + t (s < S, 256 S >= N) and owns cell t of the kConsCells cells. Dynamic LDS:
// 17 * 256 S bytes (x, y and the cell of every sorted position). Returns (thread 0's value is the
// candidate's) whether a constraint rejects the candidate.
// MOT: the motion tests (*m) beside cons7 in the loader.
template <int S, bool MOT = false, class Load>
__device__ __forceinline__ bool cons_violates(Load load, int N, const ConsArgs& a, const MotionArgs* m = nullptr)
{
    static_assert(kConsCells == kConsBlock, "one cell per thread");
    constexpr int P = kConsBlock * S;
    extern __shared__ double cons_lds[];
    double* const sx = cons_lds;
    double* const sy = cons_lds + P;
    unsigned char* const sc = reinterpret_cast<unsigned char*>(cons_lds + 2 * P);
    __shared__ double bnd[kConsCells];          // cell c holds the x with bnd[c] <= x (< bnd[c + 1])
    __shared__ int cnt[kConsCells];             // per cell: its count, then its fill cursor
    __shared__ int start[kConsCells + 1];       // first sorted position of each cell; [cells]: the total
    __shared__ double wmin[kConsBlock / kWave], wmax[kConsBlock / kWave];
    __shared__ int wsum[kConsBlock / kWave];
    __shared__ int viol;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double inf = __builtin_inf();
    if (tid == 0) viol = 0;
    cnt[tid] = 0;
    double kx[S], ky[S];
    bool bad = false;
    double lo = inf, hi = -inf;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = s * kConsBlock + tid;
        kx[s] = inf;   // +inf: not a UAV of the pair tests (past N, or a non-finite coordinate)
        ky[s] = 0.0;
        if (e < N) {
            double x, y, r;
            load(e, x, y, r);
            bad |= a.zone && y < a.zone_y && r > a.zone_r;
            if constexpr (MOT) bad |= motion_rejects(*m, e, N, x, y, r);
            if (__builtin_fabs(x) < inf && __builtin_fabs(y) < inf) {
                kx[s] = x;
                ky[s] = y;
                lo = x < lo ? x : lo;
                hi = x > hi ? x : hi;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double l2 = __shfl_xor(lo, off, kWave), h2 = __shfl_xor(hi, off, kWave);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) {
        wmin[wave] = lo;
        wmax[wave] = hi;
    }
    __syncthreads();   // (viol = 0 and cnt = 0 are visible from here on)
    if (bad) viol = 1;
#pragma unroll
    for (int q = 0; q < kConsBlock / kWave; ++q) {
        lo = wmin[q] < lo ? wmin[q] : lo;
        hi = wmax[q] > hi ? wmax[q] : hi;
    }
    // cells of width w >= dcut over [lo, hi]; bnd is non-decreasing in the cell index (the product
    // and the sum round monotonically), bnd[0] = lo. w = +inf (no cut, or an overflowing extent)
    // puts every UAV into cell 0: all pairs are tested.
    const double ext = (hi - lo) / (double)kConsCells;
    const double w = a.dcut > ext ? a.dcut : ext;
    const double invw = 1.0 / w;
    bnd[tid] = tid == 0 ? lo : lo + (double)tid * w;
    __syncthreads();
    const bool sweep = a.sep && N > 1 && !viol && lo < inf;   // workgroup-uniform
    if (sweep) {
        // each UAV's cell: a guess from the division, then corrected against the boundaries
        // themselves, so that bnd[g] <= x holds exactly, whatever the guess was
        int g[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            g[s] = -1;
            if (kx[s] < inf) {
                const double u = (kx[s] - lo) * invw;
                int q = u >= (double)(kConsCells - 1) ? kConsCells - 1 : u > 0.0 ? (int)u : 0;
                while (q > 0 && kx[s] < bnd[q]) --q;
                while (q < kConsCells - 1 && kx[s] >= bnd[q + 1]) ++q;
                g[s] = q;
                atomicAdd(&cnt[q], 1);
            }
        }
        __syncthreads();
        // exclusive scan of the counts: start[c]
        const int mine = cnt[tid];
        int incl = mine;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int v = __shfl_up(incl, off, kWave);
            if (lane >= off) incl += v;
        }
        if (lane == kWave - 1) wsum[wave] = incl;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int q = 0; q < kConsBlock / kWave; ++q) {
            base += q < wave ? wsum[q] : 0;
            total += wsum[q];
        }
        start[tid] = base + incl - mine;
        cnt[tid] = base + incl - mine;   // the cell's fill cursor
        if (tid == 0) start[kConsCells] = total;
        __syncthreads();
        // counting sort: every finite UAV takes one slot of its cell (their order inside a cell
        // depends on the atomics' order; the result, an OR over pairs, does not)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (g[s] >= 0) {
                const int pos = atomicAdd(&cnt[g[s]], 1);
                sx[pos] = kx[s];
                sy[pos] = ky[s];
                sc[pos] = (unsigned char)g[s];
            }
        }
        __syncthreads();
        const int nv = start[kConsCells];
        volatile int* const vflag = &viol;
        for (int p = tid; p < nv; p += kConsBlock) {
            if (*vflag) break;   // another thread found a violation: the candidate is decided
            const double xi = sx[p], yi = sy[p];
            int cell = sc[p];
            for (int q = p + 1; q < nv; ++q) {
                const int cq = sc[q];
                if (cq != cell) {   // a later cell: everything from here on has x >= bnd[cq]
                    if (bnd[cq] - xi >= a.dcut) break;
                    cell = cq;
                }
                const double dx = sx[q] - xi;
                if (__builtin_fabs(dx) >= a.dcut) continue;
                const double dy = sy[q] - yi;
                if (dx * dx + dy * dy <= a.T) {
                    *vflag = 1;
                    break;
                }
                if ((q & 63) == 0 && *vflag) break;
            }
        }
        __syncthreads();
    }
    return viol != 0;
}

// Workgroup = candidate (column k of the 3N x K matrix).
template <int S>
__global__ __launch_bounds__(kConsBlock) void cons_mask_kernel(const double* __restrict__ cands, int N,
                                                             ConsArgs a, uint8_t* __restrict__ feasible)
{
    const double* __restrict__ c = cands + (size_t)blockIdx.x * (size_t)(3 * N);
    const bool v = cons_violates<S>(
        [&](int e, double& x, double& y, double& r) {
            x = c[e];
            y = c[N + e];
            r = c[2 * N + e];
        },
        N, a);
    if (threadIdx.x == 0) feasible[blockIdx.x] = v ? 0 : 1;
}

// The same under a mac_motion. SEP: cons8 is on (the sort and its dynamic LDS); else motion_violates.
template <int S, bool SEP>
__global__ __launch_bounds__(kConsBlock) void cons_mask_motion_kernel(const double* __restrict__ cands, int N,
                                                                    ConsArgs a, MotionArgs m,
                                                                    uint8_t* __restrict__ feasible)
{
    const double* __restrict__ c = cands + (size_t)blockIdx.x * (size_t)(3 * N);
    auto load = [&](int e, double& x, double& y, double& r) {
        x = c[e];
        y = c[N + e];
        r = c[2 * N + e];
    };
    bool v;
    if constexpr (SEP)
        v = cons_violates<S, true>(load, N, a, &m);
    else
        v = motion_violates<S>(load, N, a, m);
    if (threadIdx.x == 0) feasible[blockIdx.x] = v ? 0 : 1;
}

// The mask over a generated poll (the native MADS driver, k_prep.h CandSrc): workgroup = candidate k
// of the source (a rank's shard: candidate src.k0 + k of the poll), its x and y drawn through
// src.get, r only under cons7. One byte per candidate of the shard, read by the poll's prep launch
// (PrepArgs.mask8). In the pipelined loop the step comes from the device state, and once the loop
// has stopped the launch returns without writing (uniform per workgroup, before any barrier).
template <int S>
__global__ __launch_bounds__(kConsBlock) void cons_mask_gen_kernel(uint64_t* ts, CandSrc src, int N, ConsArgs a,
                                                                 uint8_t* __restrict__ feasible)
{
    ts_begin(ts);   // profiling only (k_common.h)
    if (src.resolve(true)) {
        const int k = (int)blockIdx.x;
        const bool v = cons_violates<S>(
            [&](int e, double& x, double& y, double& r) {
                x = src.get(k, e, N);
                y = src.get(k, N + e, N);
                r = a.zone ? src.get(k, 2 * N + e, N) : 0.0;
            },
            N, a);
        if (threadIdx.x == 0) feasible[k] = v ? 0 : 1;
    }
    ts_end(ts);
}

// The same under a mac_motion: r is drawn under cons5, cons6 or cons7.
template <int S, bool SEP>
__global__ __launch_bounds__(kConsBlock) void cons_mask_gen_motion_kernel(uint64_t* ts, CandSrc src, int N,
                                                                        ConsArgs a, MotionArgs m,
                                                                        uint8_t* __restrict__ feasible)
{
    ts_begin(ts);   // profiling only (k_common.h)
    if (src.resolve(true)) {
        const int k = (int)blockIdx.x;
        const bool need_r = a.zone | m.speed | m.accel;
        auto load = [&](int e, double& x, double& y, double& r) {
            x = src.get(k, e, N);
            y = src.get(k, N + e, N);
            r = need_r ? src.get(k, 2 * N + e, N) : 0.0;
        };
        bool v;
        if constexpr (SEP)
            v = cons_violates<S, true>(load, N, a, &m);
        else
            v = motion_violates<S>(load, N, a, m);
        if (threadIdx.x == 0) feasible[k] = v ? 0 : 1;
    }
    ts_end(ts);
}

// ------------------------------------------------------------------ verdicts (mac_verdict, include/maxcover.h)
// What rejected a candidate: every constraint that is on is evaluated for every candidate and kept
// apart per kind, where the masks above stop at the first rejection. Kind q's bit is set exactly when
// the existing code rejects the candidate under that constraint alone, because the tests are the
// existing ones: cons3 is the prep launches' pen_term / pen_threshold (k_prep.h), cons7 zone_rejects,
// cons4 / cons5 / cons6 motion_rejects with one flag on, cons8 the pair predicate of the header under
// the same sort and the same cull. All outputs are integers (counts and lowest indices), so no order
// of threads or atomics shows in them.
//
// cons8 here counts where cons_violates stops: the sweep runs to the end, whatever the per-UAV tests
// found. The cull's proof (the header, 1-3) does not depend on stopping early: a pair that is skipped,
// alone or as the rest of a run from cell c on, is proven feasible, and every other unordered pair of
// finite UAVs is tested once, from its lower sorted position. So the number of tested pairs that
// satisfy a <= T is the number of violating pairs exactly, and a UAV is in a violating pair iff one
// of the tests it took part in (as either end) succeeded. Each sorted position carries its UAV's
// index (uint16: N <= 2048) and an "in a pair" byte that either end may set to 1: a same-value race
// in LDS, read after a barrier. Dynamic LDS: 20 * 256 S bytes (x, y, index, cell, byte).
constexpr int kVerdictKinds = 6;
enum VerdictKind { kKindCons3 = 0, kKindCons8 = 1, kKindCons7 = 2, kKindCons4 = 3, kKindCons5 = 4, kKindCons6 = 5 };
constexpr int kVerdictTally = 2 + kVerdictKinds;   // candidates, rejected by any, rejected by kind q

struct Verdict {   // mac_verdict
    uint32_t reasons;
    int32_t pairs;
    int32_t n_uav[kVerdictKinds];
    int32_t first_uav[kVerdictKinds];
    int32_t reserved[2];
};
static_assert(sizeof(Verdict) == 64, "one 64-byte record per candidate");

struct ExplainArgs {
    ConsArgs a;      // cons8, cons7
    MotionArgs m;    // cons4, cons5, cons6 (every flag 0: off, the arrays unread)
    PenArgs pa;      // cons3: prev (null: off), dlimT, tan_half_fov; rmax null
};

// One candidate by one workgroup, as cons_violates takes it. Thread 0 writes *out; tally (the
// generated-poll kernel; null: none) takes one add per non-zero term.
template <int S, bool SEP, class Load>
__device__ __forceinline__ void cons_explain(Load load, int N, const ExplainArgs& xa, Verdict* out,
                                             unsigned long long* tally)
{
    static_assert(kConsCells == kConsBlock, "one cell per thread");
    constexpr int P = kConsBlock * S;
    constexpr int NW = kConsBlock / kWave;
    constexpr int kNone = 0x7fffffff;
    __shared__ int wcnt[NW][kVerdictKinds], wfirst[NW][kVerdictKinds], wpairs[NW];
    const ConsArgs& a = xa.a;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double inf = __builtin_inf();
    // motion_rejects with one constraint on: the kind's own verdict
    MotionArgs m4 = xa.m, m5 = xa.m, m6 = xa.m;
    m4.speed = m4.accel = 0;
    m5.cone = m5.accel = 0;
    m6.cone = m6.speed = 0;
    int cnt[kVerdictKinds], first[kVerdictKinds];   // of this wave (uniform)
#pragma unroll
    for (int q = 0; q < kVerdictKinds; ++q) {
        cnt[q] = 0;
        first[q] = kNone;
    }
    double kx[S], ky[S];
    double lo = inf, hi = -inf;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = s * kConsBlock + tid;
        kx[s] = inf;   // +inf: not a UAV of the pair tests (past N, or a non-finite coordinate)
        ky[s] = 0.0;
        bool f[kVerdictKinds] = {false, false, false, false, false, false};
        if (e < N) {
            double x, y, r;
            load(e, x, y, r);
            if (xa.pa.prev) f[kKindCons3] = pen_term(x, y, r, e, N, xa.pa, pen_threshold(xa.pa, e)) < 0.0;
            f[kKindCons7] = zone_rejects(a, y, r);
            if (xa.m.cone) f[kKindCons4] = motion_rejects(m4, e, N, x, y, r);
            if (xa.m.speed) f[kKindCons5] = motion_rejects(m5, e, N, x, y, r);
            if (xa.m.accel) f[kKindCons6] = motion_rejects(m6, e, N, x, y, r);
            if (__builtin_fabs(x) < inf && __builtin_fabs(y) < inf) {
                kx[s] = x;
                ky[s] = y;
                lo = x < lo ? x : lo;
                hi = x > hi ? x : hi;
            }
        }
        // (every lane arrives here; the slots go up in e, so a wave's first hit is its lowest index)
#pragma unroll
        for (int q = 0; q < kVerdictKinds; ++q) {
            if (q == kKindCons8) continue;
            const uint64_t b = __ballot(f[q]);
            if (b != 0 && first[q] == kNone) first[q] = s * kConsBlock + wave * kWave + __builtin_ctzll(b);
            cnt[q] += __popcll(b);
        }
    }
    int pairs = 0;
    if constexpr (SEP) {
        extern __shared__ double cons_lds[];
        double* const sx = cons_lds;
        double* const sy = cons_lds + P;
        uint16_t* const si = reinterpret_cast<uint16_t*>(cons_lds + 2 * P);   // the position's UAV
        unsigned char* const sc = reinterpret_cast<unsigned char*>(si + P);   // its cell
        unsigned char* const sp = sc + P;                                     // 1: in a violating pair
        __shared__ double bnd[kConsCells];
        __shared__ int ccnt[kConsCells];
        __shared__ int start[kConsCells + 1];
        __shared__ double wmin[NW], wmax[NW];
        __shared__ int wsum[NW];
        ccnt[tid] = 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double l2 = __shfl_xor(lo, off, kWave), h2 = __shfl_xor(hi, off, kWave);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0) {
            wmin[wave] = lo;
            wmax[wave] = hi;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            lo = wmin[q] < lo ? wmin[q] : lo;
            hi = wmax[q] > hi ? wmax[q] : hi;
        }
        // the cells of cons_violates: width w >= dcut over [lo, hi], bnd non-decreasing, bnd[0] = lo
        const double ext = (hi - lo) / (double)kConsCells;
        const double w = a.dcut > ext ? a.dcut : ext;
        const double invw = 1.0 / w;
        bnd[tid] = tid == 0 ? lo : lo + (double)tid * w;
        __syncthreads();
        if (a.sep && N > 1 && lo < inf) {   // workgroup-uniform
            int g[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                g[s] = -1;
                if (kx[s] < inf) {
                    const double u = (kx[s] - lo) * invw;
                    int q = u >= (double)(kConsCells - 1) ? kConsCells - 1 : u > 0.0 ? (int)u : 0;
                    while (q > 0 && kx[s] < bnd[q]) --q;
                    while (q < kConsCells - 1 && kx[s] >= bnd[q + 1]) ++q;
                    g[s] = q;
                    atomicAdd(&ccnt[q], 1);
                }
            }
            __syncthreads();
            const int mine = ccnt[tid];
            int incl = mine;
#pragma unroll
            for (int off = 1; off < kWave; off <<= 1) {
                const int v = __shfl_up(incl, off, kWave);
                if (lane >= off) incl += v;
            }
            if (lane == kWave - 1) wsum[wave] = incl;
            __syncthreads();
            int base = 0, total = 0;
#pragma unroll
            for (int q = 0; q < NW; ++q) {
                base += q < wave ? wsum[q] : 0;
                total += wsum[q];
            }
            start[tid] = base + incl - mine;
            ccnt[tid] = base + incl - mine;   // the cell's fill cursor
            if (tid == 0) start[kConsCells] = total;
            __syncthreads();
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (g[s] >= 0) {
                    const int pos = atomicAdd(&ccnt[g[s]], 1);
                    sx[pos] = kx[s];
                    sy[pos] = ky[s];
                    si[pos] = (uint16_t)(s * kConsBlock + tid);
                    sc[pos] = (unsigned char)g[s];
                    sp[pos] = 0;
                }
            }
            __syncthreads();
            const int nv = start[kConsCells];
            // the sweep of cons_violates, to the end: every tested pair that violates is counted once
            for (int p = tid; p < nv; p += kConsBlock) {
                const double xi = sx[p], yi = sy[p];
                int cell = sc[p];
                bool hit = false;
                for (int q = p + 1; q < nv; ++q) {
                    const int cq = sc[q];
                    if (cq != cell) {   // a later cell: everything from here on has x >= bnd[cq]
                        if (bnd[cq] - xi >= a.dcut) break;
                        cell = cq;
                    }
                    const double dx = sx[q] - xi;
                    if (__builtin_fabs(dx) >= a.dcut) continue;
                    const double dy = sy[q] - yi;
                    if (dx * dx + dy * dy <= a.T) {
                        ++pairs;
                        hit = true;
                        sp[q] = 1;
                    }
                }
                if (hit) sp[p] = 1;
            }
            __syncthreads();   // (the bytes, whichever end set them)
            int c8 = 0, f8 = kNone;
            for (int p = tid; p < nv; p += kConsBlock) {
                if (sp[p]) {
                    const int e = si[p];
                    ++c8;
                    f8 = e < f8 ? e : f8;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                pairs += __shfl_xor(pairs, off, kWave);
                c8 += __shfl_xor(c8, off, kWave);
                const int o = __shfl_xor(f8, off, kWave);
                f8 = o < f8 ? o : f8;
            }
            cnt[kKindCons8] = c8;
            first[kKindCons8] = f8;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kVerdictKinds; ++q) {
            wcnt[wave][q] = cnt[q];
            wfirst[wave][q] = first[q];
        }
        wpairs[wave] = pairs;
    }
    __syncthreads();
    if (tid == 0) {
        Verdict v;
        v.reasons = 0u;
        v.pairs = 0;
#pragma unroll
        for (int q = 0; q < kVerdictKinds; ++q) {
            int c = 0, fi = kNone;
#pragma unroll
            for (int wv = 0; wv < NW; ++wv) {
                c += wcnt[wv][q];
                fi = wfirst[wv][q] < fi ? wfirst[wv][q] : fi;
            }
            v.n_uav[q] = c;
            v.first_uav[q] = c ? fi : -1;
            v.reasons |= c ? 1u << q : 0u;
        }
#pragma unroll
        for (int wv = 0; wv < NW; ++wv) v.pairs += wpairs[wv];
        v.reserved[0] = v.reserved[1] = 0;
        *out = v;
        if (tally) {   // integer adds: the totals are the same in any order
            atomicAdd(&tally[0], 1ull);
            if (v.reasons) atomicAdd(&tally[1], 1ull);
#pragma unroll
            for (int q = 0; q < kVerdictKinds; ++q)
                if (v.reasons >> q & 1u) atomicAdd(&tally[2 + q], 1ull);
        }
    }
}

// Workgroup = candidate (column k of the 3N x K matrix). SEP: cons8 is on (the sort and its dynamic LDS).
template <int S, bool SEP>
__global__ __launch_bounds__(kConsBlock) void cons_explain_kernel(const double* __restrict__ cands, int N,
                                                                ExplainArgs xa, Verdict* __restrict__ out)
{
    const double* __restrict__ c = cands + (size_t)blockIdx.x * (size_t)(3 * N);
    cons_explain<S, SEP>(
        [&](int e, double& x, double& y, double& r) {
            x = c[e];
            y = c[N + e];
            r = c[2 * N + e];
        },
        N, xa, out + blockIdx.x, nullptr);
}

// The verdicts of a generated poll (the native MADS driver under MAC_OPT_VERDICTS): workgroup =
// candidate k of the source, drawn as cons_mask_gen_motion_kernel draws it; the record into the
// launch's own scratch and the context's tally. Enqueued behind the poll's prep launch: in the
// pipelined loop the launch returns (uniform per workgroup, before any barrier) once the loop has
// stopped or when the prep rejected the poll whole, and tallies nothing then.
template <int S, bool SEP>
__global__ __launch_bounds__(kConsBlock) void cons_explain_gen_kernel(uint64_t* ts, CandSrc src, int N,
                                                                    ExplainArgs xa, Verdict* __restrict__ out,
                                                                    unsigned long long* tally)
{
    ts_begin(ts);   // profiling only (k_common.h); the driver passes null
    if (src.resolve()) {
        const int k = (int)blockIdx.x;
        const bool need_r = xa.a.zone | xa.m.speed | xa.m.accel | (xa.pa.prev != nullptr);
        cons_explain<S, SEP>(
            [&](int e, double& x, double& y, double& r) {
                x = src.get(k, e, N);
                y = src.get(k, N + e, N);
                r = need_r ? src.get(k, 2 * N + e, N) : 0.0;
            },
            N, xa, out + k, tally);
    }
    ts_end(ts);
}

// The masked poll's last launch, one workgroup: obj[k] <- +inf where feasible[k] == 0 (in place),
// then the lexicographic (objective, index) minimum over the candidates with an objective < +inf
// (finalize_argmin's rule, k_final.h: NaN and +inf never win, ties to the lowest index; none:
// {+inf, -1}), written to best and to its mapped host slot exactly as best_reduce_kernel does.
__global__ __launch_bounds__(kConsArgminBlock) void cons_argmin_kernel(double* __restrict__ obj,
                                                                     const uint8_t* __restrict__ feasible,
                                                                     int64_t K, int64_t idx_base,
                                                                     unsigned long long* best, uint64_t* mirror,
                                                                     uint64_t seq)
{
    __shared__ double wv[kConsArgminBlock / kWave];
    __shared__ long long wi[kConsArgminBlock / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double inf = __builtin_inf();
    double bv = inf;
    long long bi = -1;
    auto take = [&](double o, long long i) {
        if (i >= 0 && (bi < 0 || o < bv || (o == bv && i < bi))) {
            bv = o;
            bi = i;
        }
    };
    for (int64_t k = tid; k < K; k += kConsArgminBlock) {
        double o = obj[k];
        if (!feasible[k]) {
            o = inf;
            obj[k] = inf;
        }
        if (o < inf) take(o, (long long)k);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(bv, off, kWave);
        const long long i = __shfl_xor(bi, off, kWave);
        take(o, i);
    }
    if (lane == 0) {
        wv[wave] = bv;
        wi[wave] = bi;
    }
    __syncthreads();
    if (wave != 0) return;
    bv = lane < kConsArgminBlock / kWave ? wv[lane] : inf;
    bi = lane < kConsArgminBlock / kWave ? wi[lane] : -1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(bv, off, kWave);
        const long long i = __shfl_xor(bi, off, kWave);
        take(o, i);
    }
    if (lane == 0) {
        const bool none = bi < 0;
        const uint64_t o = __builtin_bit_cast(uint64_t, none ? inf : bv);
        const uint64_t ix = (uint64_t)(none ? (long long)-1 : (long long)idx_base + bi);
        __hip_atomic_store(best, (unsigned long long)o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(best + 1, (unsigned long long)ix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (mirror) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            mirror[0] = o;
            mirror[1] = ix;
            mirror[2] = seq;
            mirror[3] = mirror_check(o, ix, seq);
        }
    }
}

}  // namespace mac
