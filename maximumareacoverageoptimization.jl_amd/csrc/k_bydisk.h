// k_bydisk.h — per-disk attribution of one candidate's coverage in ONE launch: for every disk i
// the weight it owns (entries whose first covering disk in index order is i — the credits the
// reference's first-hit `break` loop sums, src/AreaCoverageCalculation.jl:67-78) and the weight
// it alone covers (entries no other disk covers: area(all) - area(all but i)).
//
// Shaped like closure_kernel (k_closure.h): wave w of workgroup b = disk 4b + w of candidate
// blockIdx.y, the candidate's N disks staged in dynamic LDS, the disk's tile-span row runs loaded
// in one round trip (spans of more than 64 rows walk row by row). Disk i's neighbour list has two
// sides, each compacted by ballot with its own capacity: the lower-index disks that may share an
// entry with it (they decide ownership) and the higher-index ones (they, with the lower ones,
// decide exclusivity); a side that overflows tests every disk of that side. Per entry of the span
// that disk i covers: covered by a lower neighbour -> neither; else owned, and exclusive when no
// upper neighbour covers it. Equal weights: integer counts (exact in any order); else fp64 sums in
// a fixed order (lane-strided, then the fixed butterfly) — the same order closure_kernel credits
// disk i in, so the owned values are its credits bit for bit.
//
// Each output word has one writer (lane 0 of the disk's wave): plain stores, no atomics. The area
// (nullable) is the sum of the owned values by the workgroup that arrives last: over the counts
// when the weights are equal ((sum of counts) * w0, the closure's value bit for bit), else in
// closure_kernel's fixed order. The hand-off is the closure's: thread 0 publishes its workgroup's
// owned words with agent-scope stores, drains them, then adds to the arrival counter.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "predicate.h"
#include "k_common.h"
#include "k_closure.h"

#pragma clang fp contract(off)

namespace mac {

constexpr int kByDiskNbr = 64;   // neighbours kept per side (more: every disk of that side)

struct ByDiskOut {
    double* owned;              // [K][N] (nullable)
    double* exclusive;          // [K][N] (nullable)
    double* area;               // [K] (nullable: no hand-off then)
    unsigned long long* part;   // [K][N] scratch: disk's owned count, or its owned sum's bits
    unsigned* arrive;           // [K] arrival counters, zero between launches
};

__global__ __launch_bounds__(kBlock) void by_disk_kernel(uint64_t* ts, const double* cand, int N,
                                                         Grid g, const double2* __restrict__ xy,
                                                         const double* __restrict__ w,
                                                         const int32_t* __restrict__ off, int counts,
                                                         double w0, ByDiskOut o)
{
    ts_begin(ts);
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    double* sx = (double*)lds_raw;
    double* sy = sx + N;
    double* sr = sy + N;
    // [0, kByDiskNbr): lower-index neighbours; [kByDiskNbr, 2 kByDiskNbr): higher-index ones
    __shared__ int nb[kClosureDisksPerWG][2 * kByDiskNbr];
    __shared__ double nT[kClosureDisksPerWG][2 * kByDiskNbr];
    __shared__ int rs[kClosureDisksPerWG][kWave], rpre[kClosureDisksPerWG][kWave + 1];
    __shared__ unsigned long long wown[kClosureDisksPerWG];
    __shared__ int sarr;
    {   // grid.y: the candidate
        const size_t b = blockIdx.y;
        cand += b * 3 * (size_t)N;
        if (o.owned) o.owned += b * (size_t)N;
        if (o.exclusive) o.exclusive += b * (size_t)N;
        if (o.area) o.area += b;
        o.part += b * (size_t)N;
        o.arrive += b;
    }
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int i = blockIdx.x * kClosureDisksPerWG + wid;   // this wave's disk
    const bool valid = i < N;                                // (wave-uniform)
    for (int j = tid; j < N; j += kBlock) {
        sx[j] = cand[j];
        sy[j] = cand[N + j];
        sr[j] = cand[2 * N + j];
    }
    __syncthreads();
    double cx = 0.0, cy = 0.0, r = 0.0, T = -1.0;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    bool any = false;
    if (valid) {
        cx = sx[i];
        cy = sy[i];
        r = sr[i];
        T = cover_threshold(r);
        any = T >= 0.0 && tile_span(cx, r, g.gx0, g.invS, g.nTx, x0, x1) &&
              tile_span(cy, r, g.gy0, g.invS, g.nTy, y0, y1);
    }
    // the span's row runs: lane = row, the offsets in flight during the neighbour tests
    const int nrows = any ? y1 - y0 + 1 : 0;
    const bool flat = nrows <= kWave;
    int rs0 = 0, rlen = 0;
    if (any && flat && lane < nrows) {
        const int64_t rb = (int64_t)(y0 + lane) * g.nTx;
        rs0 = off[rb + x0];
        rlen = off[rb + x1 + 1] - rs0;
    }
    // disk i's neighbours, each side compacted by ballot (list order is irrelevant: an OR)
    int nlo = 0, nhi = 0;
    if (any) {
        for (int j0 = 0; j0 < i; j0 += kWave) {
            const int j = j0 + lane;
            const bool hit = j < i && sr[j] > 0.0 && disks_may_overlap(cx, cy, r, sx[j], sy[j], sr[j]);
            const uint64_t bal = __ballot(hit);
            const int q = nlo + __popcll(bal & ((1ull << lane) - 1));
            if (hit && q < kByDiskNbr) nb[wid][q] = j;
            nlo += __popcll(bal);
        }
        for (int j0 = i + 1; j0 < N; j0 += kWave) {
            const int j = j0 + lane;
            const bool hit = j < N && sr[j] > 0.0 && disks_may_overlap(cx, cy, r, sx[j], sy[j], sr[j]);
            const uint64_t bal = __ballot(hit);
            const int q = nhi + __popcll(bal & ((1ull << lane) - 1));
            if (hit && q < kByDiskNbr) nb[wid][kByDiskNbr + q] = j;
            nhi += __popcll(bal);
        }
    }
    if (any && flat) {
        const int incl = wave_incl_scan_i32(rlen, lane);
        if (lane < nrows) rs[wid][lane] = rs0;
        rpre[wid][lane + 1] = incl;
        if (lane == 0) rpre[wid][0] = 0;
    }
    __syncthreads();
    if (any && lane < min(nlo, kByDiskNbr)) nT[wid][lane] = cover_threshold(sr[nb[wid][lane]]);
    if (any && lane < min(nhi, kByDiskNbr))
        nT[wid][kByDiskNbr + lane] = cover_threshold(sr[nb[wid][kByDiskNbr + lane]]);
    __syncthreads();
    uint64_t cnt_o = 0, cnt_x = 0;
    double acc_o = 0.0, acc_x = 0.0;
    // entry j, if disk i covers it: owned when no lower-index disk covers it, then exclusive when
    // no higher-index disk does either
    auto credit = [&](int j) {
        const double2 p = xy[j];
        if (!(sqdist(p.x, p.y, cx, cy) <= T)) return;
        bool alone = true;
        if (nlo <= kByDiskNbr) {
            for (int q = 0; q < nlo && alone; ++q) {
                const int c2 = nb[wid][q];
                alone = !(sqdist(p.x, p.y, sx[c2], sy[c2]) <= nT[wid][q]);
            }
        } else {   // overflowed list: every lower-index disk
            for (int c2 = 0; c2 < i && alone; ++c2)
                alone = !(sqdist(p.x, p.y, sx[c2], sy[c2]) <= cover_threshold(sr[c2]));
        }
        if (!alone) return;
        double wj = 0.0;
        ++cnt_o;
        if (!counts) {
            wj = w[j];
            acc_o += wj;
        }
        if (nhi <= kByDiskNbr) {
            for (int q = 0; q < nhi && alone; ++q) {
                const int c2 = nb[wid][kByDiskNbr + q];
                alone = !(sqdist(p.x, p.y, sx[c2], sy[c2]) <= nT[wid][kByDiskNbr + q]);
            }
        } else {   // overflowed list: every higher-index disk
            for (int c2 = i + 1; c2 < N && alone; ++c2)
                alone = !(sqdist(p.x, p.y, sx[c2], sy[c2]) <= cover_threshold(sr[c2]));
        }
        if (alone) {
            ++cnt_x;
            if (!counts) acc_x += wj;
        }
    };
    if (any && flat) {
        const int total = rpre[wid][nrows];
        for (int f = lane; f < total; f += kWave) {
            int lo = 0, hi = nrows - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (rpre[wid][mid] <= f) lo = mid; else hi = mid - 1;
            }
            credit(rs[wid][lo] + (f - rpre[wid][lo]));
        }
    } else if (any) {
        for (int ty = y0; ty <= y1; ++ty) {
            const int64_t rowbase = (int64_t)ty * g.nTx;
            const int s0 = off[rowbase + x0], e0 = off[rowbase + x1 + 1];
            for (int j = s0 + lane; j < e0; j += kWave) credit(j);
        }
    }
    // disk i's two values (every lane of the wave takes part in the reductions)
    double vo, vx;
    unsigned long long obits;
    if (counts) {
#pragma unroll
        for (int off2 = 32; off2 >= 1; off2 >>= 1) {
            cnt_o += __shfl_xor(cnt_o, off2, kWave);
            cnt_x += __shfl_xor(cnt_x, off2, kWave);
        }
        vo = (double)cnt_o * w0;
        vx = (double)cnt_x * w0;
        obits = cnt_o;
    } else {
        vo = wave_sum_f64(acc_o);   // (fixed butterfly)
        vx = wave_sum_f64(acc_x);
        obits = __builtin_bit_cast(unsigned long long, vo);
    }
    if (lane == 0) {
        wown[wid] = obits;
        if (valid) {
            if (o.owned) o.owned[i] = vo;
            if (o.exclusive) o.exclusive[i] = vx;
        }
    }
    if (!o.area) {   // (uniform) no area asked for
        ts_end(ts);
        return;
    }
    // the area: thread 0 publishes the workgroup's owned words (agent-scope stores, drained before
    // the one counter add), the workgroup that arrives last sums all N
    __syncthreads();
    if (tid == 0) {
        const int nw = min(kClosureDisksPerWG, N - (int)blockIdx.x * kClosureDisksPerWG);
        for (int q = 0; q < nw; ++q)
            __hip_atomic_store(o.part + blockIdx.x * kClosureDisksPerWG + q, wown[q], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        sarr = (int)__hip_atomic_fetch_add(o.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if ((unsigned)sarr != gridDim.x - 1) {   // uniform: not the last workgroup
        ts_end(ts);
        return;
    }
    __shared__ double dred[kWavesPerBlock];
    __shared__ unsigned long long cred[kWavesPerBlock];
    double area;
    if (counts) {   // integer sum: exact in any order
        uint64_t c = 0;
        for (int j = tid; j < N; j += kBlock)
            c += __hip_atomic_load(o.part + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int off2 = 32; off2 >= 1; off2 >>= 1) c += __shfl_xor(c, off2, kWave);
        if (lane == 0) cred[wid] = c;
        __syncthreads();
        uint64_t tot = 0;
#pragma unroll
        for (int q = 0; q < kWavesPerBlock; ++q) tot += cred[q];
        area = (double)tot * w0;
    } else {        // disk order per thread, then thread order (closure_kernel's)
        double a = 0.0;
        for (int j = tid; j < N; j += kBlock)
            a += __builtin_bit_cast(double, __hip_atomic_load(o.part + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        area = block_sum_f64(a, dred);   // valid in thread 0
    }
    if (tid == 0) {
        __hip_atomic_store(o.arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.area[0] = area;
    }
    ts_end(ts);
}

}  // namespace mac
