// k_prog.h — the progressive constraints of src/TDM_Constraints.jl:182-220 on the device: the
// constraint violation h of every candidate of a source (mac_prog, include/maxcover.h; the rule is
// DESIGN.md section 4 "Progressive barrier").
//
//   t_i = max(R_i - limit_i, 0.0)   Julia's max: a NaN difference stays NaN
//   c_j = sum of t_i over the UAVs i with bit j of member[i], folded from 0.0 in the order
//         i = 0, 1, ..., N-1 (src/TDM_Constraints.jl:186-190)
//   h   = sum_j c_j * c_j, folded from 0.0 in the order j = 0 .. J-1, each product rounded before
//         its add (contraction is off)
//
// A partial sum is +0.0, positive or NaN, so adding +0.0 for a UAV that is not a member (or whose
// term is +0.0) leaves it as it is, bit for bit: the fold selects the term or +0.0 and never
// branches. Workgroup = candidate. The terms of a block of kProgU UAVs are computed in parallel
// into LDS (only rows 2N .. 3N-1 of the candidate are read); lane j of wave 0 then folds constraint
// j's chain over the block in order, one lane per (candidate, constraint) chain as the prep launch
// folds the penalty (k_prep.h), and carries its partial sum to the next block. No floating-point
// atomics: every sum has one order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_common.h"
#include "k_prep.h"
#include "prog_rule.h"

#pragma clang fp contract(off)

namespace mac {

constexpr int kProgMaxN = 2048;   // UAVs under a mac_prog
constexpr int kProgMaxJ = 32;     // constraints: a bit each in member[i]
constexpr int kProgU = 512;       // UAVs per block (the prep's kPrepU)
constexpr int kProgBlock = 256;

struct ProgArgs {
    const uint32_t* member;   // N words
    const double* limit;      // N doubles
    int J;
};

// h of candidate blockIdx.x of the source (a matrix, or a generated poll around any centre
// src.xinc: shard offset, xy-only polls and the mesh through src.get, as cons_mask_gen_kernel reads
// it) into h_out[k]. mask8 (null: none): the poll's feasibility byte of the candidate, 0 when h is
// NaN or h > h_max; and_mask != 0 keeps a 0 an earlier launch on the stream (the swarm / motion
// mask) wrote there, else the byte is written.
__global__ __launch_bounds__(kProgBlock) void prog_h_kernel(uint64_t* ts, CandSrc src, int N, ProgArgs p,
                                                          double h_max, double* __restrict__ h_out,
                                                          uint8_t* __restrict__ mask8, int and_mask)
{
    __shared__ double st[kProgU];
    __shared__ uint32_t sm[kProgU];
    __shared__ double sc[kProgMaxJ];
    ts_begin(ts);   // profiling only (k_common.h)
    if (src.resolve(true)) {
        const int tid = threadIdx.x;
        const int k = (int)blockIdx.x;
        double c = 0.0;   // lane j < J of wave 0: constraint j's partial sum
        for (int u0 = 0; u0 < N; u0 += kProgU) {
            const int nb = N - u0 < kProgU ? N - u0 : kProgU;
            for (int e = tid; e < nb; e += kProgBlock) {
                const int i = u0 + e;
                const double d = src.get(k, 2 * N + i, N) - p.limit[i];
                st[e] = (d > 0.0 || d != d) ? d : 0.0;
                sm[e] = p.member[i];
            }
            __syncthreads();
            if (tid < p.J) {
                for (int e = 0; e < nb; ++e) {
                    const double t = st[e];   // (one address for the wave: an LDS broadcast)
                    c = c + (((sm[e] >> tid) & 1u) ? t : 0.0);
                }
            }
            __syncthreads();
        }
        if (tid < p.J) sc[tid] = c;
        __syncthreads();
        if (tid == 0) {
            double h = 0.0;
            for (int j = 0; j < p.J; ++j) {
                const double q = sc[j] * sc[j];
                h = h + q;
            }
            h_out[k] = h;
            if (mask8) {
                const uint8_t ok = (h != h || h > h_max) ? 0 : 1;
                mask8[k] = and_mask ? (uint8_t)(mask8[k] & ok) : ok;
            }
        }
    }
    ts_end(ts);
}

// ------------------------------------------------------------------ the barrier's update
// Steps 3-7 of the rule over the polls of one iteration: up to two centres (the feasible incumbent
// F, then the infeasible one I), K candidates each; candidate k of centre c has the global index
// g = c K + k, which orders as (centre, k) does. A candidate the chain did not evaluate (dropped by
// a mask, by cons3 or by the barrier) carries the objective +inf; a NaN objective is counted as
// evaluated and selects nothing. One workgroup, two reduction passes with a barrier between them:
// the improving case needs h_new (the largest h below I.h) before it can pick the new I. Every
// reduction is a minimum or maximum under a total order (ties to the lower g), so its result does
// not depend on the order the lanes combine in.
constexpr int kProgSelBlock = 256;

struct ProgSelArgs {
    const double* obj[2];   // per centre: K objectives, K h values (null: the centre was not polled)
    const double* h[2];
    int K;
    int has_F, has_I;
    double F_f, I_f, I_h, h_max;
};

// (ProgRec, the 64-byte record the host reads once per iteration, and prog_less2 / prog_less3: prog_rule.h)

__global__ __launch_bounds__(kProgSelBlock) void prog_select_kernel(uint64_t* ts, ProgSelArgs a,
                                                                  ProgRec* __restrict__ rec)
{
    constexpr int W = kProgSelBlock / kWave;
    __shared__ double s_f[W], s_h[W], s_hm[W];
    __shared__ long long s_g[W];
    __shared__ int s_dom[W], s_cnt[W];
    ts_begin(ts);   // profiling only (k_common.h)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const double inf = __builtin_inf();
    const int64_t total = 2 * (int64_t)a.K;
    // pass 1: the best feasible candidate, the dominating test, the largest h below I.h, the count
    double bf = inf, hm = -1.0;   // (hm < 0: no infeasible candidate below I.h; every h here is > 0)
    long long bg = -1;
    int dom = 0, cnt = 0;
    for (int64_t g = tid; g < total; g += kProgSelBlock) {
        const int c = g >= a.K ? 1 : 0;
        if (!a.obj[c]) continue;
        const int k = (int)(g - (int64_t)c * a.K);
        const double f = a.obj[c][k];
        if (f == inf) continue;   // not evaluated
        ++cnt;
        if (f != f) continue;
        const double h = a.h[c][k];
        if (h == 0.0) {
            if (prog_less2(f, g, bf, bg)) {
                bf = f;
                bg = g;
            }
        } else if (h > 0.0 && a.has_I) {
            dom |= (h <= a.I_h && f <= a.I_f && (h < a.I_h || f < a.I_f)) ? 1 : 0;
            if (h < a.I_h && h > hm) hm = h;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double f2 = __shfl_xor(bf, off, kWave);
        const long long g2 = __shfl_xor(bg, off, kWave);
        const double h2 = __shfl_xor(hm, off, kWave);
        dom |= __shfl_xor(dom, off, kWave);
        cnt += __shfl_xor(cnt, off, kWave);
        if (prog_less2(f2, g2, bf, bg)) {
            bf = f2;
            bg = g2;
        }
        hm = h2 > hm ? h2 : hm;
    }
    if (lane == 0) {
        s_f[wave] = bf;
        s_g[wave] = bg;
        s_hm[wave] = hm;
        s_dom[wave] = dom;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    bf = inf;
    bg = -1;
    hm = -1.0;
    dom = 0;
    cnt = 0;
#pragma unroll
    for (int q = 0; q < W; ++q) {   // (every thread: the values are workgroup-uniform from here on)
        if (prog_less2(s_f[q], s_g[q], bf, bg)) {
            bf = s_f[q];
            bg = s_g[q];
        }
        hm = s_hm[q] > hm ? s_hm[q] : hm;
        dom |= s_dom[q];
        cnt += s_cnt[q];
    }
    const bool improves = bg >= 0 && (!a.has_F || bf < a.F_f);
    const bool dominating = improves || dom != 0;
    const bool improving = !dominating && a.has_I && hm > 0.0;
    const double h_new = improving ? hm : (a.has_I ? a.I_h : a.h_max);
    __syncthreads();   // (s_f, s_g are reused below)
    // pass 2: the minimum of (f, h, g) over the infeasible candidates with h <= h_new
    double nf = inf, nh = inf;
    long long ng = -1;
    for (int64_t g = tid; g < total; g += kProgSelBlock) {
        const int c = g >= a.K ? 1 : 0;
        if (!a.obj[c]) continue;
        const int k = (int)(g - (int64_t)c * a.K);
        const double f = a.obj[c][k];
        if (f == inf || f != f) continue;
        const double h = a.h[c][k];
        if (h > 0.0 && h <= h_new && prog_less3(f, h, g, nf, nh, ng)) {
            nf = f;
            nh = h;
            ng = g;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double f2 = __shfl_xor(nf, off, kWave);
        const double h2 = __shfl_xor(nh, off, kWave);
        const long long g2 = __shfl_xor(ng, off, kWave);
        if (prog_less3(f2, h2, g2, nf, nh, ng)) {
            nf = f2;
            nh = h2;
            ng = g2;
        }
    }
    if (lane == 0) {
        s_f[wave] = nf;
        s_h[wave] = nh;
        s_g[wave] = ng;
    }
    __syncthreads();
    if (tid == 0) {
        nf = inf;
        nh = inf;
        ng = -1;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            if (prog_less3(s_f[q], s_h[q], s_g[q], nf, nh, ng)) {
                nf = s_f[q];
                nh = s_h[q];
                ng = s_g[q];
            }
        }
        // the old I stays in the running when I.h <= h_new, and sorts before a candidate on a full tie
        if (a.has_I && a.I_h <= h_new &&
            !(ng >= 0 && (nf < a.I_f || (nf == a.I_f && nh < a.I_h)))) {
            nf = a.I_f;
            nh = a.I_h;
            ng = kProgOld;
        }
        rec->outcome = (dominating ? 0 : improving ? 1 : 2) | (improves ? 256 : 0);
        rec->bestF_f = bf;
        rec->bestF_g = bg;
        rec->newI_f = nf;
        rec->newI_h = nh;
        rec->newI_g = ng;
        rec->h_new = h_new;
        rec->evaluated = cnt;
    }
    ts_end(ts);
}

// ------------------------------------------------------------------ the barrier's update, one shard
// The shard-partial record of prog_rule.h over one shard of an iteration's polls: per centre c the Kc
// candidates lo .. lo + Kc - 1 of its K (objectives and h as the chain and prog_h_kernel left them for
// the shard; null: the centre was not polled), global index g = c K + lo + k. One workgroup, one pass:
// every thread folds its strided candidates (prog_part_fold), the waves merge by shuffles, the four
// wave records meet in LDS and thread 0 writes the 96 bytes. Every field merges under a total order,
// so the record does not depend on the order the lanes combine in. No atomics, no second pass.
constexpr int kProgPartBlock = 256;

struct ProgPartArgs {
    const double* obj[2];
    const double* h[2];
    int Kc, K;
    int64_t lo, tag;
    ProgScalars s;
};

__device__ __forceinline__ ProgPart prog_part_shfl(const ProgPart& p, int off)
{
    ProgPart q;
    q.tag = p.tag;
    q.evaluated = __shfl_xor((long long)p.evaluated, off, kWave);
    q.bestF_f = __shfl_xor(p.bestF_f, off, kWave);
    q.bestF_g = __shfl_xor((long long)p.bestF_g, off, kWave);
    q.dominates = __shfl_xor((int)p.dominates, off, kWave);
    q.h_below = __shfl_xor(p.h_below, off, kWave);
    q.keep_f = __shfl_xor(p.keep_f, off, kWave);
    q.keep_h = __shfl_xor(p.keep_h, off, kWave);
    q.keep_g = __shfl_xor((long long)p.keep_g, off, kWave);
    q.drop_f = __shfl_xor(p.drop_f, off, kWave);
    q.drop_h = __shfl_xor(p.drop_h, off, kWave);
    q.drop_g = __shfl_xor((long long)p.drop_g, off, kWave);
    return q;
}

__global__ __launch_bounds__(kProgPartBlock) void prog_part_kernel(uint64_t* ts, ProgPartArgs a,
                                                                   ProgPart* __restrict__ out)
{
    constexpr int W = kProgPartBlock / kWave;
    __shared__ ProgPart s_part[W];
    ts_begin(ts);   // profiling only (k_common.h)
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    ProgPart p = prog_part_empty(a.tag);
    const int64_t total = 2 * (int64_t)a.Kc;
    for (int64_t e = tid; e < total; e += kProgPartBlock) {
        const int c = e >= a.Kc ? 1 : 0;
        if (!a.obj[c]) continue;
        const int k = (int)(e - (int64_t)c * a.Kc);
        const double f = a.obj[c][k];
        if (f == __builtin_inf()) continue;   // (not evaluated: its h may never have been written)
        prog_part_fold(p, a.s, f, a.h[c][k], (int64_t)c * a.K + a.lo + k);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const ProgPart q = prog_part_shfl(p, off);
        prog_part_merge(p, q);
    }
    if (lane == 0) s_part[wave] = p;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int q = 1; q < W; ++q) prog_part_merge(p, s_part[q]);
        *out = p;
    }
    ts_end(ts);
}

}  // namespace mac
