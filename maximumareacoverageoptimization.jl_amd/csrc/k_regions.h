// k_regions.h — high-interest regions (src/FullSimulation.jl:751-754): axis-aligned boxes over the
// fire-point list.
//
// Membership is the reference's own test (src/CellFunctions.jl:42, :68; src/FullSimulation.jl:542):
//     x < x_UB && x > x_LB && y < y_UB && y > y_LB        (fp64, all strict; NaN anywhere: false)
// so an entry with a non-finite coordinate is in no box, and neither is anything in a box with
// lb >= ub or a NaN bound.
//
//   region_ingest_kernel  one pass over the entries that just arrived in the list ([lo, hi) of the
//                         list-order arrays): an entry inside any box gets the high-interest weight
//                         (the override at push!, :42-45 / :68-72) and is counted per box and once
//                         for the union. Lane b of a wave keeps box b's count in a register (wave
//                         ballots), the block adds its waves' counts in LDS: one integer atomic per
//                         workgroup per box.
//   region_stats_kernel   the CURRENT list through the tile index. The key is ty * nTx + tx, so a
//                         box's part of one tile row is the contiguous run off[ty*nTx + tile_of(x_LB)]
//                         .. off[ty*nTx + tile_of(x_UB) + 1] (tile_of is monotone: a superset; every
//                         entry is still decided by the four compares). A wave takes one item
//                         (box, band of tile rows, chunk of each row's run) and writes its partial
//                         counts and weights; an entry counts for the union in its lowest-index box
//                         (the exactly-once rule the disks use), and such an entry is covered when
//                         one of the disks that can reach the item's tiles (culled into LDS by
//                         tile_span) has sqdist <= T, the coverage predicate itself.
//   region_reduce_kernel  adds the items' partials in item order, one workgroup per box and one for
//                         the union: no floating-point atomics, the same bits on every run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "predicate.h"
#include "k_common.h"

#pragma clang fp contract(off)

namespace mac {

constexpr int kRegionsMax = 64;          // MAC_REGIONS_MAX: one lane of a wave per box
constexpr int kRegMaxDisks = 2048;       // disks of a covered query (their indices fit the LDS lists)
constexpr int kRegIngestBlocks = 1024;   // grid-stride cap of the ingest launch
constexpr int kRegItemCap = 65536;       // items of one stats call (40 B of partials each)
constexpr int kRegChunk = 512;           // entries an item aims at

static_assert(kRegionsMax == kWave, "lane b counts box b");

// bounds layout (device and LDS): [x_LB | x_UB | y_LB | y_UB], kRegionsMax doubles each
__device__ __forceinline__ bool in_box(double x, double y, const double* B, int b)
{
    return x < B[kRegionsMax + b] && x > B[b] && y < B[3 * kRegionsMax + b] && y > B[2 * kRegionsMax + b];
}

// counts: [0, kRegionsMax) per box, [kRegionsMax] the union
__global__ __launch_bounds__(kBlock) void region_ingest_kernel(
    const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ w, int64_t lo,
    int64_t hi, const double* __restrict__ boxes, int nb, double w_high, int set_weight,
    unsigned long long* __restrict__ counts)
{
    __shared__ double B[4 * kRegionsMax];
    __shared__ unsigned wc[kWavesPerBlock][kRegionsMax + 1];
    for (int q = threadIdx.x; q < 4 * kRegionsMax; q += kBlock) B[q] = boxes[q];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    unsigned mine = 0;   // lane b: this wave's entries inside box b
    unsigned anyc = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t base = lo + (int64_t)blockIdx.x * kBlock + wid * kWave; base < hi; base += stride) {
        const int64_t i = base + lane;
        const bool live = i < hi;
        const double px = live ? x[i] : __builtin_nan(""), py = live ? y[i] : __builtin_nan("");
        bool any = false;
        for (int b = 0; b < nb; ++b) {   // (uniform: every lane votes)
            const bool in = live && in_box(px, py, B, b);
            const unsigned long long m = __ballot(in);
            if (lane == b) mine += (unsigned)__popcll(m);
            any |= in;
        }
        if (any) {
            ++anyc;
            if (set_weight) w[i] = w_high;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) anyc += __shfl_xor(anyc, o, kWave);
    wc[wid][lane] = mine;
    if (lane == 0) wc[wid][kRegionsMax] = anyc;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < nb || t == kRegionsMax) {
        unsigned long long s = 0;
#pragma unroll
        for (int q = 0; q < kWavesPerBlock; ++q) s += wc[q][t];
        if (s) atomicAdd(&counts[t], s);
    }
}

// One box's items: nrg bands of G tile rows (from ty0) x nch chunks of every row's run; the items
// base .. base + nrg * nch - 1 (band-major). nrg = 0: the box holds nothing (lb >= ub, NaN bound).
struct RegItem {
    int tx0, tx1, ty0, ty1;
    int G, nch, nrg, base;
};

struct RegPartial {
    double w, anyw, covw;
    unsigned cnt, anycnt, covcnt, box;
};

__global__ __launch_bounds__(kBlock) void region_stats_kernel(
    const double2* __restrict__ xys, const double* __restrict__ ws, const int32_t* __restrict__ off, Grid g,
    const double* __restrict__ boxes, int nb, const RegItem* __restrict__ items, int total,
    const DiskRec* __restrict__ disks, int N, RegPartial* __restrict__ part)
{
    __shared__ double B[4 * kRegionsMax];
    __shared__ RegItem IT[kRegionsMax];
    __shared__ uint16_t dl[kWavesPerBlock][kRegMaxDisks];
    for (int q = threadIdx.x; q < 4 * kRegionsMax; q += kBlock) B[q] = boxes[q];
    for (int q = threadIdx.x; q < nb; q += kBlock) IT[q] = items[q];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int item = (int)blockIdx.x * kWavesPerBlock + wid;
    const bool valid = item < total;   // (wave-uniform; an idle wave only meets the barrier below)
    int b = 0, rA = 0, rB = -1, c = 0;
    RegItem I{};
    if (valid) {
        for (int q = 0; q < nb; ++q)
            if (IT[q].nrg > 0 && item >= IT[q].base) b = q;   // bases ascend over the boxes with items
        I = IT[b];
        const int local = item - I.base;
        const int rg = local / I.nch;
        c = local - rg * I.nch;
        rA = I.ty0 + rg * I.G;
        rB = min(rA + I.G - 1, I.ty1);
    }
    // the disks that can cover an entry of this item's tiles
    int nd = 0;
    if (valid) {
        for (int c0 = 0; c0 < N; c0 += kWave) {
            const int k = c0 + lane;
            bool keep = false;
            if (k < N) {
                int4 sp;
                keep = disk_span(disks[k], g, sp) && sp.x <= I.tx1 && sp.y >= I.tx0 && sp.z <= rB &&
                       sp.w >= rA;
            }
            const unsigned long long m = __ballot(keep);
            if (keep) dl[wid][nd + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)k;
            nd += __popcll(m);
        }
    }
    __syncthreads();
    if (!valid) return;
    double sw = 0.0, sa = 0.0, sc = 0.0;
    unsigned nw = 0, na = 0, nc = 0;
    for (int ty = rA; ty <= rB; ++ty) {
        const int64_t rowbase = (int64_t)ty * g.nTx;
        const int64_t s = off[rowbase + I.tx0], e = off[rowbase + I.tx1 + 1];
        const int64_t len = e - s;
        const int64_t j0 = s + len * c / I.nch, j1 = s + len * (c + 1) / I.nch;
        for (int64_t j = j0 + lane; j < j1; j += kWave) {
            const double2 p = xys[j];
            if (!in_box(p.x, p.y, B, b)) continue;
            const double wv = ws[j];
            ++nw;
            sw += wv;
            bool first = true;   // the union credits the lowest-index box holding the entry
            for (int q = 0; q < b; ++q)
                if (in_box(p.x, p.y, B, q)) {
                    first = false;
                    break;
                }
            if (!first) continue;
            ++na;
            sa += wv;
            for (int q = 0; q < nd; ++q) {
                const DiskRec d = disks[dl[wid][q]];
                if (sqdist(p.x, p.y, d.cx, d.cy) <= d.T) {
                    ++nc;
                    sc += wv;
                    break;
                }
            }
        }
    }
    sw = wave_sum_f64(sw);
    sa = wave_sum_f64(sa);
    sc = wave_sum_f64(sc);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        nw += __shfl_xor(nw, o, kWave);
        na += __shfl_xor(na, o, kWave);
        nc += __shfl_xor(nc, o, kWave);
    }
    if (lane == 0) {
        RegPartial P;
        P.w = sw;
        P.anyw = sa;
        P.covw = sc;
        P.cnt = nw;
        P.anycnt = na;
        P.covcnt = nc;
        P.box = (unsigned)b;
        part[item] = P;
    }
}

// Workgroup b < nb: box b's count and weight into oc[b], ow[b]; workgroup nb: the union's into
// [nb] and the covered part of it into [nb + 1]. Each thread adds every kBlock-th item of its range
// in ascending order, then the fixed butterfly and the waves in order.
__global__ __launch_bounds__(kBlock) void region_reduce_kernel(const RegPartial* __restrict__ part,
                                                               const RegItem* __restrict__ items, int nb,
                                                               int total, unsigned long long* __restrict__ oc,
                                                               double* __restrict__ ow)
{
    __shared__ double sd[2][kWavesPerBlock];
    __shared__ unsigned long long si[2][kWavesPerBlock];
    const int b = blockIdx.x;
    const bool uni = b == nb;
    int lo = 0, hi = total;
    if (!uni) {
        const RegItem I = items[b];
        lo = I.base;
        hi = I.nrg > 0 ? I.base + I.nrg * I.nch : I.base;
    }
    double d0 = 0.0, d1 = 0.0;
    unsigned long long i0 = 0, i1 = 0;
    for (int q = lo + (int)threadIdx.x; q < hi; q += kBlock) {
        const RegPartial P = part[q];
        if (uni) {
            d0 += P.anyw;
            d1 += P.covw;
            i0 += P.anycnt;
            i1 += P.covcnt;
        } else {
            d0 += P.w;
            i0 += P.cnt;
        }
    }
    d0 = wave_sum_f64(d0);
    d1 = wave_sum_f64(d1);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        i0 += __shfl_xor(i0, o, kWave);
        i1 += __shfl_xor(i1, o, kWave);
    }
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    if (lane == 0) {
        sd[0][wid] = d0;
        sd[1][wid] = d1;
        si[0][wid] = i0;
        si[1][wid] = i1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a0 = 0.0, a1 = 0.0;
        unsigned long long c0 = 0, c1 = 0;
#pragma unroll
        for (int q = 0; q < kWavesPerBlock; ++q) {
            a0 += sd[0][q];
            a1 += sd[1][q];
            c0 += si[0][q];
            c1 += si[1][q];
        }
        oc[b] = c0;
        ow[b] = a0;
        if (uni) {
            oc[nb + 1] = c1;
            ow[nb + 1] = a1;
        }
    }
}

}  // namespace mac
