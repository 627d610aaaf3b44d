// k_prep.h — the prep launch (penalty chains, fp32 keys, per-disk range records) and the scan's disk records.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "predicate.h"
#include "mesh_key.h"
#include "mads_walk.h"
#include "k_common.h"

#pragma clang fp contract(off)

namespace mac {

// ------------------------------------------------------------------ per-batch disk prep

// Objective-penalty inputs (src/TDM_STATIC_opt.jl:89-97) and the cons3 constraint
// (src/TDM_Constraints.jl:54-75). rmax == null: no penalty term; prev == null: no cons3.
struct PenArgs {
    const double* rmax;
    const double* prev;
    const double* dlimT;   // per UAV: cons3 holds iff s <= dlimT[i] (predicate.h dlim_threshold)
    const double* dlim;    // ... or the raw d_lim[i], thresholded where it is read (dlimT == null)
    double tan_half_fov;
};

// UAV i's cons3 threshold: dlimT[i], or dlim_threshold(d_lim[i]) (evaluated once per disk by the
// callers that loop over candidates, so the device API needs no threshold launch of its own)
__device__ __forceinline__ double pen_threshold(const PenArgs& pa, int i)
{
    if (!pa.prev) return 0.0;
    return pa.dlimT ? pa.dlimT[i] : dlim_threshold(pa.dlim[i]);
}

// Term i of candidate (x_i, y_i, R_i): |R_i - rmax_i| (0 without rmax), or -1 when UAV i's move
// violates cons3 (sqrt(dx^2 + dy^2 + dz^2) > d_lim[i], z = R / tan(FOV/2), evaluated exactly as
// s > T3 = pen_threshold(pa, i)). A negative term marks the candidate infeasible; the finalize
// chain sums the others sequentially in i (bit-exact with the reference's loop).
__device__ __forceinline__ double pen_term(double x2, double y2, double R2, int i, int N,
                                           const PenArgs& pa, double T3)
{
    if (pa.prev) {
        const double x1 = pa.prev[i], y1 = pa.prev[N + i], z1 = pa.prev[2 * N + i] / pa.tan_half_fov;
        const double z2 = R2 / pa.tan_half_fov;
        const double ddx = x1 - x2, ddy = y1 - y2, ddz = z1 - z2;
        const double s = ddx * ddx + ddy * ddy + ddz * ddz;
        if (s > T3) return -1.0;
    }
    return pa.rmax ? __builtin_fabs(R2 - pa.rmax[i]) : 0.0;
}

// Whether UAV i's diagonal LTMADS steps reject every candidate that carries them: with the
// incumbent's value v of one of UAV i's variables (q = 0 x, 1 y, 2 r), both v + b and v - b (b =
// 2^ell; the generator's x +- entry with entry = +-b gives exactly these doubles) put that
// variable's own term of cons3's sum above T3. The sum dx^2 + dy^2 + dz^2 in floating point is at
// least each of its terms (adding non-negative terms is monotone under rounding), so the whole
// candidate fails cons3 then, whatever its other entries. Every variable is the diagonal of one
// column of B, so when this holds for all 3N variables no candidate of the poll passes cons3.
// pen_term's arithmetic (x1 - x2, z = R / tan(FOV/2), z1 - z2).
__host__ __device__ __forceinline__ bool diag_rejects(double v, double b, double p, int q,
                                                      double tan_half_fov, double T3)
{
    bool all = true;
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
        const double c = sg == 0 ? v + b : v - b;
        double d;
        if (q < 2) {
            d = p - c;
        } else {
            const double z1 = p / tan_half_fov, z2 = c / tan_half_fov;
            d = z1 - z2;
        }
        const double sq = d * d;
        all = all && sq > T3;
    }
    return all;
}

// ------------------------------------------------------------------ candidate sources

// (the stream's draws, splitmix_at / ltmads_entry: mads_walk.h)

// The native MADS loop's state on the device when its polls are pipelined (mads_driver.h
// mads_run_pipelined): the finalize of poll t applies poll t's update (k_final.h mads_step) and
// poll t + 1's launches read the mesh index from here, so the host enqueues polls ahead of their
// outcomes. ell < 0 (the mesh precision limit) stops the loop: every later launch returns at once.
// A poll that cons3 rejects whole (skip = 1, written by the poll's prep launch: every variable's
// diagonal step ±2^ell alone violates its UAV's d_lim, k_prep.h poll_rejected) is a failure with
// no evaluation: the launches after the prep return at once and the finalize applies the failure
// update. feas counts the candidates that pass cons3 (the evaluations the reference makes).
struct MadsState {
    double f;      // objective at the incumbent
    int64_t it;    // polls applied
    int ell;       // mesh index of the next poll (step 2^ell)
    int skip;      // the current poll is rejected whole (set by its prep launch)
    unsigned long long feas;   // candidates evaluated (passing cons3)
    int64_t skipped;           // polls rejected whole
    int64_t succ;              // successful polls (the incumbent moved)
    const double* gran;        // the mesh's granularity per variable (CandSrc.mesh below; null: none)
};

// Where candidate coordinates come from: a 3N x K column-major matrix (the batch APIs), or a
// complete LTMADS poll around an incumbent generated on the fly (the native MADS driver):
// candidate k < n is x + B[:, k], k >= n is x - B[:, k - n], B = L[rp][:, cp] (variable v of a
// candidate = x_i for v = i, y_i for v = N + i, r_i for v = 2N + i). An xy-only poll (MAC_POLL_XY:
// src/TDM_STATIC_opt.jl:15-44) draws its basis over the n_p = 2N variables x_0.., y_0.. alone: 2 n_p
// candidates, split at n_p, every candidate's radii the incumbent's doubles as they are.
struct CandSrc {
    const double* cands;   // matrix source when non-null
    int ldc;
    const uint32_t* keysP; // packed integer keys, one row per disk (the prep launch), when non-null
    const float* keysT;    // ... and the fp32 keys of the escaped values, variable-major rows
    int ldk;               // row pitch of both (keys_ld(K))
    const double* xinc;    // generator: incumbent (3N), row / column permutations (n each)
    const int* rp;
    const int* cp;
    uint64_t state;
    int64_t b;             // 2^ell
    int k0;                // generator: candidate k of this source is candidate k0 + k of the poll
                           // (a rank's shard of it)
    int np;                // generator: polled variables n_p, the first n_p of x (0: all 3N)
    const MadsState* mst;  // generator, pipelined MADS loop: b from the device state (else null)
    // the basis form (mac_poll_basis_f64: a caller-owned poll, DirectSearch's B = L[rp][:, cp] and
    // mesh size delta, src/TDM_STATIC_opt.jl:22-44): L's lower triangle packed by rows (int16,
    // entry (r, c <= r) at r(r+1)/2 + c) and B's entries delta * L instead of the stream's draws
    // (null: the stream). b is then a bound on |L| (the index's int16 table) and delta scales it.
    // On the stream (ltri null) delta's eight bytes hold the native MADS driver's mesh instead
    // (mac_mads_mesh; set_mesh / mesh below): the device pointer to the granularity g of every
    // variable (3N doubles; null, delta's 0.0: 1.0 everywhere, the draws as they are). Variable v's
    // step is fl(g[v] * entry): one product (step below). One slot for both, so the launches'
    // arguments keep their size (a larger CandSrc costs prep_x_kernel's matrix build two spills).
    const int16_t* ltri;
    double delta;
    // (host only) the chain a generated poll takes under MAC_CHAIN_AUTO: 1 = the five-launch chain
    // (the host found the poll crowded: maxcover.hip host_crowded_disks), 0 = AUTO's history
    int route_five;
    // (host only, in the struct's tail padding) a generated poll on a mesh keys its disks in mesh units
    // (MAC_OPT_MESH_KEYS, mesh_key.h): the chains' kMesh == kMeshKeys builds
    int mesh_keys;
    // Called at the top of every launch that reads the source: b = 2^ell from the device state;
    // false once the loop has stopped, or (launches after the prep: any_poll false) when the
    // prep rejected the poll whole (the launch returns at once). Uniform per workgroup.
    __device__ __forceinline__ bool resolve(bool any_poll = false)
    {
        if (!mst) return true;
        const int e = mst->ell;
        if (e < 0 || (!any_poll && mst->skip)) return false;
        b = (int64_t)1 << e;
        return true;
    }
    // polled variables of a generated poll over N UAVs
    __host__ __device__ __forceinline__ int polled(int N) const { return np ? np : 3 * N; }
    // B's entry (r, c) of a generated poll (n = n_p): the stream's LTMADS draw, or delta * L[r][c]
    __device__ __forceinline__ double entry(int n, int r, int c) const
    {
        if (ltri) return r < c ? 0.0 : delta * (double)ltri[(int64_t)r * (r + 1) / 2 + c];
        return ltmads_entry(state, n, b, r, c);
    }
    // (through an integer: a cast of the double's bits straight to a pointer went through the stack)
    __host__ __device__ __forceinline__ const double* mesh_ptr() const
    {
        return reinterpret_cast<const double*>(__builtin_bit_cast(uint64_t, delta));
    }
    __host__ __device__ __forceinline__ const double* mesh() const { return ltri ? nullptr : mesh_ptr(); }
    __host__ void set_mesh(const double* g)   // (ltri null)
    {
        delta = __builtin_bit_cast(double, reinterpret_cast<uint64_t>(g));
    }
    // Polled variable v's step of B's entry (r, c): the entry, times the variable's granularity on
    // a mesh (without a mesh the entry itself, not a product by 1.0). kM selects the mesh at compile
    // time for the launches of the poll chains, whose no-mesh builds are the code they were (kNoMesh;
    // kOnMesh: the host selects it when mesh() is set), or tests the pointer (kAnyMesh: the mask, the
    // identity index and the streaming scan's records).
    static constexpr int kNoMesh = 0, kOnMesh = 1, kAnyMesh = 2;
    template <int kM> __device__ __forceinline__ double step_m(int n, int v, int r, int c) const
    {
        const double d = entry(n, r, c);
        if constexpr (kM == kNoMesh) return d;
        else if constexpr (kM == kOnMesh) return mesh_ptr()[v] * d;
        else {
            const double* g = mesh();
            return g ? g[v] * d : d;
        }
    }
    // variable v's diagonal step at mesh step b = 2^ell (the whole-poll rejection, diag_rejects)
    template <int kMesh> __device__ __forceinline__ double diag_step(int v, double b) const
    {
        if constexpr (kMesh != 0) return mesh_ptr()[v] * b;
        else return b;
    }
    // a full poll's value (np == 0), for the launches that select the poll kind at compile time
    // (the disk index: its full-poll instantiation is the code it was)
    template <int kM> __device__ __forceinline__ double get_full_m(int kl, int v, int N) const
    {
        if (cands) return cands[(int64_t)kl * ldc + v];
        const int n = 3 * N;
        const int k = kl + k0;
        const int kk = k < n ? k : k - n;
        const double d = step_m<kM>(n, v, rp[v], cp[kk]);
        return k < n ? xinc[v] + d : xinc[v] - d;
    }
    __device__ __forceinline__ double get(int kl, int v, int N) const { return get_m<kAnyMesh>(kl, v, N); }
    template <int kM> __device__ __forceinline__ double get_m(int kl, int v, int N) const
    {
        if (cands) return cands[(int64_t)kl * ldc + v];
        const int n = polled(N);
        const int k = kl + k0;
        const int kk = k < n ? k : k - n;
        // (selects, no branch: the loads stay independent of the compare and issue together; a held
        // variable, v >= n under an xy-only poll, reads row 0 and keeps x's double as it is, no + 0.0)
        const bool held = v >= n;
        const double xv = xinc[v];
        const double d = step_m<kM>(n, held ? 0 : v, rp[held ? 0 : v], cp[kk]);
        const double moved = k < n ? xv + d : xv - d;
        return held ? xv : moved;
    }
    // The source selected at compile time (the fused chain's second and third launches, k_fiw.h):
    // kMat is a matrix source, read from cands alone — no generator code in that instantiation and
    // none of its operands held in registers — and never paused by a device state (no mst).
    template <bool kMat, int kMesh = 0> __device__ __forceinline__ double val(int kl, int v, int N) const
    {
        if constexpr (kMat) return cands[(int64_t)kl * ldc + v];
        else return cands ? cands[(int64_t)kl * ldc + v] : get_m<kMesh ? kOnMesh : kNoMesh>(kl, v, N);
    }
    // Mesh keys (mesh_key.h): a generated candidate's value as get_m<kOnMesh> builds it, and in e the
    // signed draw behind it (+-entry, the integer the stream drew; 0.0 for a held variable)
    __device__ __forceinline__ double get_draw(int kl, int v, int N, double& e) const
    {
        const int n = polled(N);
        const int k = kl + k0;
        const int kk = k < n ? k : k - n;
        const bool held = v >= n;
        const double xv = xinc[v];
        const double en = entry(n, rp[held ? 0 : v], cp[kk]);
        const double d = mesh_ptr()[held ? 0 : v] * en;
        const double moved = k < n ? xv + d : xv - d;
        e = held ? 0.0 : k < n ? en : -en;
        return held ? xv : moved;
    }
    template <bool kMat> __device__ __forceinline__ bool resolve_as()
    {
        if constexpr (kMat) return true;
        else return resolve();
    }
};

static_assert(sizeof(CandSrc) == 120, "the launches' arguments keep their size");

// ------------------------------------------------------------------ the prep launch
// The first launch of every evaluation: workgroup cw takes candidates [8cw, 8cw + 8), thread u
// UAV u of each block of kPrepU UAVs, and reads that UAV's (x, y, r) of its 8 candidates — 24
// coalesced loads, all in flight at once — from the 3N x K matrix as Julia hands it over (or the
// LTMADS generator). The matrix is read once per evaluation, here; from those values:
//   objective (vp != null): term_i = |R_i - rmax_i|, or -1 when UAV i's move fails cons3
//     (pen_term's arithmetic), into LDS; lane c of wave 0 folds candidate 8cw + c's terms IN
//     ORDER i = 0, 1, ..., N-1 from 0.0, as src/TDM_STATIC_opt.jl:88-92 does (bit-exact): one
//     lane per chain. vp[k] = violation * penalty, or +inf when a term is negative (the extreme
//     barrier of src/TDM_Constraints.jl:54-75);
//   poll walk (prec != null): one 16-B record per (workgroup, UAV), prec[cw*N + i] (a
//     coalesced store): {x range, y range, span-area estimate, key flag}. The range is a tile box
//     containing the tile span (predicate.h tile_span) of every one of the 8 disks,
//     from min(c - r), max(c + r) and max(|c| + r) per axis: tile_span's rounding steps are
//     monotone in those, so the box bounds each span from outside (a superset region only
//     makes the walk stage or share more entries, never changes a result), packed as two
//     16-bit tile numbers (range_pack); the estimate is the disks' span areas as (2r/S + 1)^2
//     (the walk choice's cost). The disk index reduces disk i's records (k_index.h);
//   keys (keysP != null; matrix or generator): the packed key of each disk (below), relative to
//     candidate 0's, into keysP[i*ldk + k] (8 consecutive words: two 16-B stores); an escaped
//     disk's three fp32 offsets fl32(v - v0) into keysT[v*ldk + k]; the record's key flag is 1
//     when one of those does not reproduce its double bit for bit (k_index.h "Keys": the disk
//     then takes the identity map).
#ifndef MAC_PREP_C
#define MAC_PREP_C 8
#endif
constexpr int kPrepC = MAC_PREP_C;   // candidates per workgroup (a multiple of 4)
constexpr int kPrepU = 512;      // UAVs per block = threads per workgroup

// keysP / keysT row pitch: rows start on 128-B boundaries (and hold every workgroup's kPrepC keys:
// a workgroup writes kPrepC keys from k0 = its index * kPrepC, so 32 must be a multiple of kPrepC
// or the last workgroup's keys would spill into the next row); the chain fold is one wave
static_assert(kPrepC % 4 == 0 && 32 % kPrepC == 0 && kPrepC <= 64,
              "MAC_PREP_C must divide 32 and be a multiple of 4");
__host__ __device__ inline int keys_ld(int K) { return (K + 31) & ~31; }

struct PrepArgs {
    CandSrc src;
    int N, K;
    PenArgs pa;
    double penalty;
    double* vp;                // per-candidate penalty (null: no objective)
    int pair;                  // generated complete polls (K = 2n, n = n_p, n % 4 == 0): workgroup cw takes
                               // x + B[:, k] and x - B[:, k] for k in [4cw, 4cw + 4) (one draw of
                               // each B entry for both: prep_cand)
    int nchain;                // workgroups
    int skip_failed;           // 1: the records leave out cons3 failures (no area is reported for them)
    int xbase;                 // (prep_x_kernel) workgroup cw also takes candidate xbase + cw when < K
    int4* prec;                // [nchain][N] records (null: no poll walk)
    Grid g;
    uint32_t* keysP;           // packed keys (null: none), one row per disk, pitch ldk
    float* keysT;              // fp32 keys of escaped values, 3N rows of pitch ldk
    int ldk;
    // the fused chain (k_fiw.h; null: none): per workgroup the largest displacement of a disk from
    // candidate 0's over its live candidates {max |x - x0|, max |y - y0|, max r - r0, max r0 - r}
    // (keysP needed; a NaN difference counts as +inf),
    // and one byte per candidate: 1 when it fails cons3 and is left out (skip_failed, N <= kPrepU)
    double4* pd;
    uint8_t* dead8;
    // the pipelined MADS loop with cons3 (null: none): the state whose skip word this launch
    // writes (workgroup 0), the poll being rejected whole when every variable's diagonal step
    // fails (diag_rejects); then every workgroup returns before its records
    MadsState* mst_w;
    unsigned long long* feas;  // += the candidates that pass cons3 (null: not counted)
    int* lreset;               // the fused chain's hand-off list count, zeroed for this poll (null: none)
    // generated polls under swarm constraints (k_cons.h cons_mask_gen_kernel; null: none): one byte
    // per candidate of the source, 0 = rejected. A rejected candidate counts as a cons3 failure
    // (vp = +inf, not in feas; with skip_failed and N <= kPrepU in dead8 and out of the records,
    // the displacement bound and the key flag). Matrix sources do not read it. (xbase sits in
    // the padding above, so the kernel arguments keep their size.)
    const uint8_t* mask8;
};

// The candidates of a workgroup's slots the swarm mask rejects, as a bit per slot (uniform: scalar
// loads). cand(c) >= K: absent.
template <int NC, class Cand>
__device__ __forceinline__ uint32_t prep_masked(const uint8_t* mask8, int K, Cand cand)
{
    uint32_t m = 0u;
    if (mask8) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = cand(c);
            if (k < K && mask8[k] == 0) m |= 1u << c;
        }
    }
    return m;
}

// The fused chain's prep over a matrix source (prep_x_kernel): kPrepCX candidates per workgroup
// and floor(K / kPrepCX) workgroups, the remainder (fewer than the workgroups) one more each to
// the first. At config 4 (K = 3073) that is 512 workgroups, two on every CU; kPrepC = 8 gives 385,
// two on 129 CUs and one on the rest, and the doubled CUs set the launch's length.
constexpr int kPrepCX = 6;

// Packed keys. Disk i of candidate k is keyed by its offsets (dx, dy, dr) from candidate 0's
// disk. When all three are integers that reproduce the doubles exactly (v0 + (double)d == v bit
// for bit) with |dx|, |dy| <= 1023 and |dr| <= 511 — every MADS poll on the granular mesh up to
// step 2^9 — the key is one 32-bit word (11 + 11 + 10 bits, two's complement); else the word is
// the escape kKeyEsc (r field -512) and the value's three fp32 offsets go to the keysT rows
// (k_index.h "Keys"). Either encoding satisfies v == v0 + (double)key, so equal keys still mean
// equal disks; the index reads one word per candidate instead of three.
// Mesh keys (kMesh == kMeshKeys: MAC_OPT_MESH_KEYS on a generated poll with a mesh; mesh_key.h): the
// word holds the disk's signed draws (m_x, m_y, m_r) instead, base the incumbent and scale the disk's
// granularities, built from the draws the launch has in hand before the product; a draw past its
// field, or a decode that is not the double, leaves the escape word, marks the record inexact (the
// identity map) and writes no fp32 row: mesh units and metres never meet in one key space.
constexpr uint32_t kKeyEsc = 0x200u << 22;
static_assert(kKeyEsc == kMeshKeyEsc, "one escape word");
constexpr int kMeshKeys = 2;   // kMesh: 0 no mesh, 1 a mesh with value keys, 2 a mesh with mesh keys
__device__ __forceinline__ bool key_int(double v, double b, double lim, int& d)
{
    const double f = v - b;
    if (!(f >= -lim && f <= lim)) return false;   // (NaN: false)
    d = (int)f;
    return (double)d == f && __builtin_bit_cast(uint64_t, b + (double)d) == __builtin_bit_cast(uint64_t, v);
}
__device__ __forceinline__ uint32_t key_pack(int dx, int dy, int dr)
{
    return ((uint32_t)dx & 0x7FFu) | (((uint32_t)dy & 0x7FFu) << 11) | (((uint32_t)dr & 0x3FFu) << 22);
}
__device__ __forceinline__ void key_unpack(uint32_t p, float& x, float& y, float& r)
{
    x = (float)((int)(p << 21) >> 21);
    y = (float)((int)(p << 10) >> 21);
    r = (float)((int)p >> 22);
}

// the tile range [lo, hi] on one axis covering every span of disks with min(c - r) = a,
// max(c + r) = b, max(|c| + r) = m (tile_span's steps, each monotone); false: empty
__device__ __forceinline__ bool partial_range(double a, double b, double m, double g0, double invS,
                                              int n, int& lo, int& hi)
{
    const double ulo = (a - g0) * invS;
    const double uhi = (b - g0) * invS;
    const double err = (m + __builtin_fabs(g0)) * invS * 1e-14 + 1e-9;
    const double flo = __builtin_floor(ulo - err);
    const double fhi = __builtin_floor(uhi + err);
    if (!(flo == flo) || !(fhi == fhi)) { lo = 0; hi = n - 1; return true; }
    if (fhi < 0.0 || flo > (double)(n - 1)) return false;
    lo = flo < 0.0 ? 0 : (int)flo;
    hi = fhi > (double)(n - 1) ? n - 1 : (int)fhi;
    return true;
}

// A tile range [lo, hi] of an axis of n tiles as two 16-bit numbers lo >> s, hi >> s, with s the
// least shift that fits n - 1 below 0xFFFF (0 for every grid of up to 65535 tiles a side);
// unpacking rounds outwards (a superset); the empty range packs as {0xFFFF, 0}, the identity of
// the (min, max) reduction.
__host__ __device__ inline int range_shift(int n)
{
    int s = 0;
    while (((n - 1) >> s) > 0xFFFE) ++s;
    return s;
}
__device__ __forceinline__ uint32_t range_pack(bool any, int lo, int hi, int s)
{
    return any ? (uint32_t)(lo >> s) | ((uint32_t)(hi >> s) << 16) : 0xFFFFu;
}
__device__ __forceinline__ void range_unpack(uint32_t lo16, uint32_t hi16, int s, int n, int& lo, int& hi)
{
    lo = (int)(lo16 << s);
    hi = min((int)(((hi16 + 1) << s) - 1), n - 1);
}

#ifdef MAC_DIAG
__device__ uint64_t g_diag_prep[64 * 16];   // diagnostic build only: workgroup phase stamps
#define MAC_PREP_STAMP_T(q, t) if (threadIdx.x == (t) && cw < 64 && (q) < 16) g_diag_prep[16 * cw + (q)] = __builtin_amdgcn_s_memrealtime()
#else
#define MAC_PREP_STAMP_T(q, t)
#endif
#define MAC_PREP_STAMP(q) MAC_PREP_STAMP_T(q, 0)

// A workgroup barrier for LDS only: global stores still in flight are not waited for
// (__syncthreads would drain them first)
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// the workgroup's LDS (one block for both source kinds: their instantiations would each
// declare their own)
template <int PC>   // (PC: candidate slots per workgroup)
struct PrepLds {
    double term[PC][kPrepU + 2];   // [candidate][UAV]; rows 16-B aligned (the fold reads pairs),
                                   // 4 banks apart (+2)
    int wbad[kPrepU / kWave][PC];  // per wave: a term of the candidate is negative
    uint32_t wbadm[kPrepU / kWave];   // ... wbad as a mask over the candidates
    int wrej[kPrepU / kWave];         // per wave: every UAV's diagonal steps fail (mst_w)
    double dred[kPrepU / kWave][4];   // per wave: its share of the displacement bound
};

template <bool kMat, int PC, int kMesh = 0>   // (kMesh: a generated poll on a mesh, CandSrc.step_m)
__device__ __forceinline__ void prep_block(const PrepArgs& a, int cw, unsigned char* lds)
{
    constexpr int kM = kMesh ? CandSrc::kOnMesh : CandSrc::kNoMesh;
    constexpr int NC = PC;   // candidate slots
    PrepLds<NC>& L = *reinterpret_cast<PrepLds<NC>*>(lds);
    auto& term = L.term;
    auto& wbad = L.wbad;
    auto& wbadm = L.wbadm;
    auto& wrej = L.wrej;
    auto& dred = L.dred;
    const int N = a.N, K = a.K;
    const int u = threadIdx.x, lane = u & (kWave - 1), wid = u / kWave;
    const int k0 = cw * PC;
    const int np = a.src.polled(N);   // (generated polls: the polled variables, 3N or 2N)
    // candidate c of the workgroup: k0 + c, or (pairs) the plus / minus candidates of B's columns
    // [4cw, 4cw + 4): c < 4 -> 4cw + c, c >= 4 -> n + 4cw + c - 4
    auto cand = [&](int c) { return a.pair ? (c < 4 ? 4 * cw + c : np + 4 * cw + c - 4) : k0 + c; };
    const bool obj = a.vp != nullptr;
    const PenArgs& pa = a.pa;
    MAC_PREP_STAMP(0);
    double acc = 0.0;   // the chain (lane c of wave 0: candidate k0 + c)
    bool bad = false;   // ... and whether a term of it is negative (cons3)
    // Candidates that fail cons3 (the extreme barrier, src/TDM_Constraints.jl:54-75) are not
    // evaluated by the reference's DirectSearch poll, and their objective is +inf whatever they
    // cover. With one block of UAVs (N <= kPrepU) their failure is known before the records are
    // written, so the records leave them out (the regions, and with them the walks' work, shrink
    // to the feasible candidates; the index maps them to an inert position, k_index.h). Uniform.
    // (a generated poll's swarm mask joins the failures: mdead, bit c = slot c rejected)
    uint32_t mdead = 0u;
    if constexpr (!kMat) mdead = prep_masked<NC>(obj ? a.mask8 : nullptr, K, cand);
    const bool masked = !kMat && a.mask8 != nullptr;
    const bool excl = obj && (pa.prev || masked) && (a.prec || a.pd) && a.skip_failed && N <= kPrepU;
    double dmx = -__builtin_inf(), dmy = -__builtin_inf(), dmr = -__builtin_inf();   // (pd)
    double dml = -__builtin_inf();   // (pd) max r0 - r
    uint32_t dead = 0u;   // (excl) bit c: candidate c fails cons3 (0 otherwise)
    for (int ib = 0; ib < N; ib += kPrepU) {
        const int nb = min(kPrepU, N - ib);
        const int i = ib + u;
        const bool iv = u < nb;
        const int ii = min(i, N - 1);
        double v[NC][3];
        // (mesh keys) per slot its word from the draws, and a bit when it does not pack or decode
        [[maybe_unused]] uint32_t mkw[NC] = {};
        [[maybe_unused]] uint32_t mkbad = 0u;
        if (!kMat && PC == 8 && a.pair) {
            // x +- B[v][col]: each draw once for the candidate pair (PC == 8: four columns)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int col = 4 * cw + c;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int vv = q * N + ii;
                    if (q == 2 && 2 * N >= np) {   // (uniform) an xy-only poll: the radius as it is, no draw
                        v[c][q] = v[c + 4][q] = a.src.xinc[vv];
                        if constexpr (kMesh == kMeshKeys) {   // (held: m = 0)
                            const double gq = a.src.mesh_ptr()[vv];
                            mkbad |= (mesh_key_put(mkw[c], q, v[c][q], gq, 0.0, v[c][q]) ? 0u : 1u) << c;
                            mkbad |= (mesh_key_put(mkw[c + 4], q, v[c][q], gq, 0.0, v[c][q]) ? 0u : 1u) << (c + 4);
                        }
                        continue;
                    }
                    if constexpr (kMesh == kMeshKeys) {
                        const double xv = a.src.xinc[vv], gq = a.src.mesh_ptr()[vv];
                        const double e = a.src.entry(np, a.src.rp[vv], a.src.cp[col]);
                        const double d = gq * e;   // (step_m's product)
                        v[c][q] = xv + d;
                        v[c + 4][q] = xv - d;
                        mkbad |= (mesh_key_put(mkw[c], q, xv, gq, e, v[c][q]) ? 0u : 1u) << c;
                        mkbad |= (mesh_key_put(mkw[c + 4], q, xv, gq, -e, v[c + 4][q]) ? 0u : 1u) << (c + 4);
                        continue;
                    }
                    const double d = a.src.step_m<kM>(np, vv, a.src.rp[vv], a.src.cp[col]);
                    v[c][q] = a.src.xinc[vv] + d;
                    v[c + 4][q] = a.src.xinc[vv] - d;
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = min(cand(c), K - 1);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    if constexpr (kMat) v[c][q] = a.src.cands[(int64_t)k * a.src.ldc + q * N + ii];
                    else if constexpr (kMesh == kMeshKeys) {
                        const int vv = q * N + ii;
                        double e;
                        v[c][q] = a.src.get_draw(k, vv, N, e);
                        mkbad |= (mesh_key_put(mkw[c], q, a.src.xinc[vv], a.src.mesh_ptr()[vv], e, v[c][q]) ? 0u : 1u) << c;
                    } else v[c][q] = a.src.get_m<kM>(k, q * N + ii, N);
                }
            }
        }
        if constexpr (kMesh == kMeshKeys) {
            // the words leave at once (nothing here reads them back): only the escape bits stay live
            // through the fold, for the record's flag
            if (a.keysP && iv) {
                uint32_t* const krow = a.keysP + (int64_t)i * a.ldk;
#pragma unroll
                for (int h = 0; h < PC / 4; ++h) {
                    uint32_t w4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) w4[e] = ((mkbad >> (4 * h + e)) & 1u) ? kKeyEsc : mkw[4 * h + e];
                    *reinterpret_cast<uint4*>(krow + cand(4 * h)) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
                }
            }
        }
        double base[3] = {0.0, 0.0, 0.0};   // candidate 0's values: the keys' base
        // (mesh keys: the base of the fused chain's displacement bound alone)
        if (a.keysP && (kMesh != kMeshKeys || a.pd)) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if constexpr (kMat) base[q] = a.src.cands[q * N + ii];
                else base[q] = a.src.get_m<kM>(0, q * N + ii, N);
            }
        }
        if (obj) {
            // pen_term (above), the same operations in the same order
            const double x1 = pa.prev ? pa.prev[ii] : 0.0, y1 = pa.prev ? pa.prev[N + ii] : 0.0;
            const double z1 = pa.prev ? pa.prev[2 * N + ii] / pa.tan_half_fov : 0.0;
            const double rm = pa.rmax ? pa.rmax[ii] : 0.0;
            const double T3 = pen_threshold(pa, ii);
            uint32_t wdead = 0u;   // this wave's part of the failures
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double R2 = v[c][2];
                double t = pa.rmax ? __builtin_fabs(R2 - rm) : 0.0;
                if (pa.prev) {
                    const double z2 = R2 / pa.tan_half_fov;
                    const double ddx = x1 - v[c][0], ddy = y1 - v[c][1], ddz = z1 - z2;
                    const double sq = ddx * ddx + ddy * ddy + ddz * ddz;
                    if (sq > T3) t = -1.0;
                }
                term[c][u] = t;
                const uint64_t neg = __ballot(iv && t < 0.0);
                if (lane == 0) wbad[wid][c] = neg != 0;
                wdead |= (neg != 0 ? 1u : 0u) << c;
            }
            if (lane == 0) wbadm[wid] = wdead;
            if (a.mst_w) {   // (excl, one block of UAVs: uniform) the whole-poll rejection
                bool rej = true;
                if (iv) {
                    const double bb = (double)a.src.b;   // (on a mesh: variable v's step g[v] * 2^ell)
                    auto ds = [&](int v) { return a.src.diag_step<kMesh>(v, bb); };
                    rej = diag_rejects(a.src.xinc[ii], ds(ii), x1, 0, pa.tan_half_fov, T3) &&
                          diag_rejects(a.src.xinc[N + ii], ds(N + ii), y1, 1, pa.tan_half_fov, T3) &&
                          (2 * N >= np ||   // (uniform: over the polled variables only)
                           diag_rejects(a.src.xinc[2 * N + ii], ds(2 * N + ii), pa.prev[2 * N + ii], 2,
                                        pa.tan_half_fov, T3));
                }
                const uint64_t keep = __ballot(!rej);
                if (lane == 0) wrej[wid] = keep == 0;
            }
            MAC_PREP_STAMP(1 + 3 * (ib / kPrepU));
            lds_barrier();   // every wave's terms and failures
            if (excl) {   // (the records below leave the failures out)
                dead = mdead;
#pragma unroll
                for (int w = 0; w < kPrepU / kWave; ++w) dead |= wbadm[w];
                if (a.mst_w) {
                    bool rej = true;
#pragma unroll
                    for (int w = 0; w < kPrepU / kWave; ++w) rej = rej && wrej[w] != 0;
                    if (cw == 0 && u == 0) a.mst_w->skip = rej ? 1 : 0;
                    if (rej) return;   // (uniform) the later launches see skip and return
                }
            }
            if (u < NC) {
                // the chain, sequential in UAV order: lane c of wave 0 folds candidate slot c
                // while the other waves go on to the bound and the keys below (wave 0 does its own
                // share of them after the fold, which sets the launch's length)
#pragma unroll
                for (int w = 0; w < kPrepU / kWave; ++w) bad |= wbad[w][u] != 0;
                if constexpr (!kMat) bad |= ((mdead >> u) & 1u) != 0;
                if (!bad) {   // (a cons3 failure's vp is +inf: no chain to fold)
                    // the chain's wave first at issue: the dependent adds are the launch's
                    // critical path, the other waves on its SIMD have slack
                    __builtin_amdgcn_s_setprio(3);
                    // batches of 2 kB terms (pair reads), the next batch's reads in flight while
                    // this batch's adds run: the dependent adds, not the LDS latency, set the pace
                    constexpr int kB = 3;   // (the most that fits 128 VGPRs beside v)
                    const double2* row2 = reinterpret_cast<const double2*>(&term[u][0]);
                    const int nfull = nb / (2 * kB);
                    // ping-pong buffers (no register moves between batches); the reads past the
                    // last batch re-read it (clamped) and are never added
                    auto batch = [&](double2 (&buf)[kB], int bt) {
                        const int at = (bt < nfull ? bt : nfull - 1) * kB;
#pragma unroll
                        for (int j = 0; j < kB; ++j) buf[j] = row2[at + j];
                    };
                    auto add = [&](const double2 (&buf)[kB]) {
#pragma unroll
                        for (int j = 0; j < kB; ++j) {
                            acc += buf[j].x;
                            acc += buf[j].y;
                        }
                    };
                    if (nfull > 0) {
                        double2 A[kB], B[kB];
                        batch(A, 0);
#pragma unroll 1
                        for (int bt = 0; bt < nfull; bt += 2) {
                            batch(B, bt + 1);
                            __builtin_amdgcn_sched_barrier(0);   // (the reads stay ahead of the adds)
                            add(A);
                            if (bt + 1 >= nfull) break;
                            batch(A, bt + 2);
                            __builtin_amdgcn_sched_barrier(0);
                            add(B);
                        }
                    }
                    for (int q = nfull * 2 * kB; q < nb; ++q) acc += term[u][q];
                    __builtin_amdgcn_s_setprio(0);
                }
            }
            MAC_PREP_STAMP(2 + 3 * (ib / kPrepU));
        }
        if (a.pd && a.keysP && iv) {
            // the fused chain's displacement bound (k_fiw.h sup_box): over this workgroup's live
            // candidates (the ones the records below would take), a NaN difference counts as +inf
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double x = v[c][0], y = v[c][1], r = v[c][2];
                if (cand(c) < K && !((dead >> c) & 1u) && r > 0.0 && __builtin_isfinite(x) &&
                    __builtin_isfinite(y)) {
                    double ex = __builtin_fabs(x - base[0]), ey = __builtin_fabs(y - base[1]), er = r - base[2];
                    double el = base[2] - r;
                    if (!(ex <= kDblMax)) ex = __builtin_inf();
                    if (!(ey <= kDblMax)) ey = __builtin_inf();
                    if (!(er == er)) er = __builtin_inf();
                    if (!(el == el)) el = __builtin_inf();
                    dmx = fmax(dmx, ex);
                    dmy = fmax(dmy, ey);
                    dmr = fmax(dmr, er);
                    dml = fmax(dml, el);
                }
            }
        }
        if (a.pd && ib + kPrepU >= N) {   // (uniform) this wave's share of the bound, into LDS
            // (thread 0 combines the waves at the end)
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                dmx = fmax(dmx, __shfl_xor(dmx, o, kWave));
                dmy = fmax(dmy, __shfl_xor(dmy, o, kWave));
                dmr = fmax(dmr, __shfl_xor(dmr, o, kWave));
                dml = fmax(dml, __shfl_xor(dml, o, kWave));
            }
            if (lane == 0) {
                dred[wid][0] = dmx;
                dred[wid][1] = dmy;
                dred[wid][2] = dmr;
                dred[wid][3] = dml;
            }
        }
        if ((a.prec || a.keysP) && iv) {
            double xa = __builtin_inf(), xb = -__builtin_inf(), ya = __builtin_inf(), yb = -__builtin_inf();
            double xm = 0.0, ym = 0.0, est = 0.0;
            bool any = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (!a.prec) break;   // (the fused chain: keys only, no region records)
                const double x = v[c][0], y = v[c][1], r = v[c][2];
                // span_of's cases: r <= 0 or NaN, or a non-finite centre, covers nothing
                if (cand(c) < K && !((dead >> c) & 1u) && r > 0.0 && __builtin_isfinite(x) &&
                    __builtin_isfinite(y)) {
                    any = true;
                    xa = fmin(xa, x - r);
                    xb = fmax(xb, x + r);
                    ya = fmin(ya, y - r);
                    yb = fmax(yb, y + r);
                    xm = fmax(xm, __builtin_fabs(x) + r);
                    ym = fmax(ym, __builtin_fabs(y) + r);
                    const double e = 2.0 * r * a.g.invS + 1.0;
                    est += e * e;
                }
            }
            bool kb = false;   // a key of this disk is inexact (k_index.h "Keys")
            if constexpr (kMesh == kMeshKeys) {
                // (the words were stored above; no fp32 row: a live escape is the identity map)
                kb = a.keysP && (mkbad & ~dead) != 0u;
            } else if (a.keysP) {     // the keys: packed words (two 16-B stores), escapes in fp32
                uint32_t pk[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    int dx = 0, dy = 0, dr = 0;
                    const bool packs = key_int(v[c][0], base[0], 1023.0, dx) &&
                                       key_int(v[c][1], base[1], 1023.0, dy) &&
                                       key_int(v[c][2], base[2], 511.0, dr);
                    pk[c] = packs ? key_pack(dx, dy, dr) : kKeyEsc;
                    if (!packs) {
#pragma unroll
                        for (int q = 0; q < 3; ++q) {
                            const float f = (float)(v[c][q] - base[q]);
                            kb |= !((dead >> c) & 1u) && __builtin_bit_cast(uint64_t, base[q] + (double)f) != __builtin_bit_cast(uint64_t, v[c][q]);
                            a.keysT[(int64_t)(q * N + i) * a.ldk + cand(c)] = f;
                        }
                    }
                }
                uint32_t* const krow = a.keysP + (int64_t)i * a.ldk;
#pragma unroll
                for (int h = 0; h < PC / 4; ++h)   // candidates cand(4h) .. cand(4h) + 3
                    *reinterpret_cast<uint4*>(krow + cand(4 * h)) =
                        make_uint4(pk[4 * h], pk[4 * h + 1], pk[4 * h + 2], pk[4 * h + 3]);
            }
            if (a.prec) {
                int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
                any = any && partial_range(xa, xb, xm, a.g.gx0, a.g.invS, a.g.nTx, x0, x1) &&
                      partial_range(ya, yb, ym, a.g.gy0, a.g.invS, a.g.nTy, y0, y1);
                a.prec[(int64_t)cw * N + i] =
                    make_int4((int)range_pack(any, x0, x1, range_shift(a.g.nTx)),
                              (int)range_pack(any, y0, y1, range_shift(a.g.nTy)),
                              __builtin_bit_cast(int, (float)est), kb ? 1 : 0);
            }
        }
        MAC_PREP_STAMP(3 + 3 * (ib / kPrepU));
        if (obj && ib + kPrepU < N) lds_barrier();   // the fold has read the terms
    }
    if (obj && u < NC && cand(u) < K) {
        a.vp[cand(u)] = bad ? __builtin_inf() : acc * a.penalty;
        if (a.dead8) a.dead8[cand(u)] = excl && bad ? 1 : 0;
    }
    if (obj && a.feas && wid == 0) {   // the evaluations: candidates that pass cons3
        const uint64_t ok = __ballot(u < NC && cand(u) < K && !bad);
        if (lane == 0 && ok) atomicAdd(a.feas, (unsigned long long)__popcll(ok));
    }
    if (a.pd) {   // the workgroup's displacement bound: the waves' shares in order
        lds_barrier();
        if (u == 0) {
            double4 m = make_double4(dred[0][0], dred[0][1], dred[0][2], dred[0][3]);
            for (int q = 1; q < kPrepU / kWave; ++q) {
                m.x = fmax(m.x, dred[q][0]);
                m.y = fmax(m.y, dred[q][1]);
                m.z = fmax(m.z, dred[q][2]);
                m.w = fmax(m.w, dred[q][3]);
            }
            a.pd[cw] = m;
        }
    }
}

// The fused chain's prep over a matrix source with one block of UAVs (N <= kPrepU; k_fiw.h):
// kPrepCX candidates per workgroup plus, for the first K - xbase workgroups, candidate xbase + cw
// (slot kPrepCX). Waves 0..7 hold a UAV per thread: loads, penalty terms and cons3 ballots, one
// barrier, then per candidate slot the packed key and the share of the displacement bound, while
// a ninth wave that holds no UAV folds the chains (lane c: slot c's, sequential in UAV order). The
// fold and the keys are exclusive branches, so the candidate values are dead on the folding
// wave's path (80 VGPRs: two workgroups, 18 waves, fit a CU). Results are prep_block's bit for bit
// (the same terms in the same order, the same keys and bound). The matrix build's UAV waves are
// VALU-bound behind the barrier (they end after the folding wave, tools/diag_prep.py), so it does
// no arithmetic for a slot kPrepCX that holds no candidate (all but the first K - xbase workgroups)
// and takes a packed slot's share of the bound from the key's integers; the generated builds are
// the code they were.
template <bool kGen, int kMesh = 0>   // (kMesh: as prep_block's)
__device__ __forceinline__ void prep_block_x(const PrepArgs& a, int cw, unsigned char* lds)
{
    constexpr int kM = kMesh ? CandSrc::kOnMesh : CandSrc::kNoMesh;
    // kGen: a generated complete poll (K = 2n, n = 3N): workgroup cw takes the columns 3cw .. 3cw + 2
    // of B, slots 0-2 their plus candidates (k = col), slots 3-5 their minus candidates (k = n + col),
    // each B entry drawn once for both; N workgroups
    constexpr int PC = kPrepCX, NC = kGen ? kPrepCX : kPrepCX + 1, NW = kPrepU / kWave;
    PrepLds<kPrepCX + 1>& L = *reinterpret_cast<PrepLds<kPrepCX + 1>*>(lds);
    auto& term = L.term;
    auto& wbad = L.wbad;
    auto& wbadm = L.wbadm;
    auto& wrej = L.wrej;
    auto& dred = L.dred;
    const int N = a.N, K = a.K;
    const int u = threadIdx.x, lane = u & (kWave - 1), wid = u / kWave;
    const bool fw = wid == NW;   // the folding wave
    const int k0 = cw * PC;
    const int n3 = 3 * N;
    auto cand = [&](int c) {   // (>= K: absent)
        if constexpr (kGen) return c < 3 ? 3 * cw + c : n3 + 3 * cw + c - 3;
        else return c < PC ? k0 + c : a.xbase + cw;
    };
    const bool obj = a.vp != nullptr;
    const PenArgs& pa = a.pa;
    // (a generated poll's swarm mask joins the failures: mdead, bit c = slot c rejected)
    uint32_t mdead = 0u;
    if constexpr (kGen) mdead = prep_masked<NC>(obj ? a.mask8 : nullptr, K, cand);
    const bool masked = kGen && a.mask8 != nullptr;
    const bool excl = obj && (pa.prev || masked) && a.skip_failed;
    const bool iv = !fw && u < N;
    const int ii = min(u, N - 1);
    // (matrix) slot PC holds a candidate in the first K - xbase workgroups alone: the others load it
    // (clamped, so the loads issue as one straight run) and skip its arithmetic. Uniform.
    const bool has7 = kGen || cand(PC) < K;
    MAC_PREP_STAMP(0);
    double v[NC][3];
    double base[3] = {0.0, 0.0, 0.0};   // candidate 0's values: the keys' base
    // (mesh keys) per slot its word from the draws, and a bit when it does not pack or decode
    [[maybe_unused]] uint32_t mkw[NC] = {};
    [[maybe_unused]] uint32_t mkbad = 0u;
    if (!fw) {
        // The penalty's own inputs (prev, rmax, the cons3 threshold or the raw d_lim: N-sized) are
        // issued ahead of the matrix loads and first looked at behind them (the asm below), so z1
        // and the threshold are worked out while the candidates' values are in flight.
        // (Every per-UAV load below is a uniform base plus one of three 32-bit byte offsets, UAV ii's
        // x, y and r: a scalar base and a shared offset register a load, not a 64-bit address each.)
        [[maybe_unused]] const uint32_t ob[3] = {(uint32_t)ii * 8u, (uint32_t)(N + ii) * 8u,
                                                 (uint32_t)(2 * N + ii) * 8u};
        [[maybe_unused]] auto at = [](const double* p, uint32_t o) {
            return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(p) + o);
        };
        // (A generated poll issues the five together behind its draws instead, without the pins:
        // held across the generator's 64-bit arithmetic they cost every kGen build spills.)
        double p1x = 0.0, p1y = 0.0, p1r = 0.0, rm = 0.0, dl = 0.0;
        if constexpr (!kGen) {
            if (obj) {
                if (pa.prev) {
                    p1x = at(pa.prev, ob[0]);
                    p1y = at(pa.prev, ob[1]);
                    p1r = at(pa.prev, ob[2]);
                    dl = at(pa.dlimT ? pa.dlimT : pa.dlim, ob[0]);
                }
                if (pa.rmax) rm = at(pa.rmax, ob[0]);
            }
        }
        if constexpr (kGen) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int vv = q * N + ii;
                const int rv = a.src.rp[vv];
                const double xv = a.src.xinc[vv];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if constexpr (kMesh == kMeshKeys) {
                        const double gq = a.src.mesh_ptr()[vv];
                        const double e = a.src.entry(n3, rv, a.src.cp[3 * cw + c]);
                        const double d = gq * e;   // (step_m's product)
                        v[c][q] = xv + d;
                        v[c + 3][q] = xv - d;
                        mkbad |= (mesh_key_put(mkw[c], q, xv, gq, e, v[c][q]) ? 0u : 1u) << c;
                        mkbad |= (mesh_key_put(mkw[c + 3], q, xv, gq, -e, v[c + 3][q]) ? 0u : 1u) << (c + 3);
                        continue;
                    }
                    const double d = a.src.step_m<kM>(n3, vv, rv, a.src.cp[3 * cw + c]);
                    v[c][q] = xv + d;
                    v[c + 3][q] = xv - d;
                }
                if (kMesh != kMeshKeys || a.pd)   // (mesh keys: the displacement bound's base alone)
                    base[q] = xv + a.src.step_m<kM>(n3, vv, rv, a.src.cp[0]);
            }
            if constexpr (kMesh == kMeshKeys) {
                // the words leave at once: only the escape bits stay live past the barrier
                if (iv) {
                    uint32_t* const krow = a.keysP + (int64_t)u * a.ldk;
#pragma unroll
                    for (int c = 0; c < NC; ++c) krow[cand(c)] = ((mkbad >> c) & 1u) ? kKeyEsc : mkw[c];
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = min(cand(c), K - 1);
                const double* const col = a.src.cands + (int64_t)k * a.src.ldc;   // (uniform)
#pragma unroll
                for (int q = 0; q < 3; ++q) v[c][q] = at(col, ob[q]);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) base[q] = at(a.src.cands, ob[q]);
        }
        if (obj) {
            if constexpr (kGen) {
                if (pa.prev) {
                    p1x = pa.prev[ii];
                    p1y = pa.prev[N + ii];
                    p1r = pa.prev[2 * N + ii];
                    dl = pa.dlimT ? pa.dlimT[ii] : pa.dlim[ii];
                }
                if (pa.rmax) rm = pa.rmax[ii];
            }
            // The first empty asm keeps every use of the five small values below the issue of the
            // candidates' loads; the second keeps z1 and the threshold above the first use of a
            // candidate's value. The language promises neither order, so after a compiler change check
            // the ISA (make asm, or hipcc -S --offload-device-only) of prep_x_kernel<false>: the five
            // small loads, then the 21 matrix and 3 base loads stand back to back, the first wait
            // after them is counted (s_waitcnt vmcnt(24): only the small loads), the division and
            // dlim_threshold follow it, and the terms wait for the matrix in counted steps.
            if constexpr (!kGen) asm volatile("" : "+v"(p1x), "+v"(p1y), "+v"(p1r), "+v"(rm), "+v"(dl) : : "memory");
            // pen_term (above), the same operations in the same order
            const double x1 = p1x, y1 = p1y;
            double z1 = pa.prev ? p1r / pa.tan_half_fov : 0.0;
            // (pen_threshold's value: dlimT[ii], or the raw d_lim[ii] thresholded here)
            double T3 = !pa.prev ? 0.0 : pa.dlimT ? dl : dlim_threshold(dl);
            if constexpr (!kGen) asm volatile("" : "+v"(z1), "+v"(T3));
            uint32_t wdead = 0u;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if constexpr (!kGen) {
                    // an absent slot PC: no term (its row is read by no live fold lane), no failure
                    // (wbad and wbadm's bit written as 0: a dead bit must not leak into `dead`)
                    if (c == PC && !has7) {
                        if (lane == 0) wbad[wid][c] = 0;
                        continue;
                    }
                }
                const double R2 = v[c][2];
                double t = pa.rmax ? __builtin_fabs(R2 - rm) : 0.0;
                if (pa.prev) {
                    const double z2 = R2 / pa.tan_half_fov;
                    const double ddx = x1 - v[c][0], ddy = y1 - v[c][1], ddz = z1 - z2;
                    const double sq = ddx * ddx + ddy * ddy + ddz * ddz;
                    if (sq > T3) t = -1.0;
                }
                term[c][u] = t;
                const uint64_t neg = __ballot(iv && t < 0.0);
                if (lane == 0) wbad[wid][c] = neg != 0;
                wdead |= (neg != 0 ? 1u : 0u) << c;
            }
            if (lane == 0) wbadm[wid] = wdead;
            if (a.mst_w) {   // the whole-poll rejection (uniform)
                bool rej = true;
                if (iv) {
                    const double bb = (double)a.src.b;   // (on a mesh: variable v's step g[v] * 2^ell)
                    auto ds = [&](int v) { return a.src.diag_step<kMesh>(v, bb); };
                    rej = diag_rejects(a.src.xinc[ii], ds(ii), x1, 0, pa.tan_half_fov, T3) &&
                          diag_rejects(a.src.xinc[N + ii], ds(N + ii), y1, 1, pa.tan_half_fov, T3) &&
                          diag_rejects(a.src.xinc[2 * N + ii], ds(2 * N + ii), pa.prev[2 * N + ii], 2,
                                       pa.tan_half_fov, T3);
                }
                const uint64_t keep = __ballot(!rej);
                if (lane == 0) wrej[wid] = keep == 0;
            }
        }
    }
    MAC_PREP_STAMP(1);
    uint32_t dead = 0u;
    if (obj) {
        lds_barrier();   // every wave's terms and failures
        if (excl) {
            dead = mdead;
#pragma unroll
            for (int w = 0; w < NW; ++w) dead |= wbadm[w];
            if (a.mst_w) {
                bool rej = true;
#pragma unroll
                for (int w = 0; w < NW; ++w) rej = rej && wrej[w] != 0;
                if (cw == 0 && u == 0) a.mst_w->skip = rej ? 1 : 0;
                if (rej) return;   // (uniform) the later launches see skip and return
            }
        }
    }
    MAC_PREP_STAMP(2);
    if (fw) {   // the chains
        bool bad = false;
        double acc = 0.0;
        if (obj && lane < NC) {
#pragma unroll
            for (int w = 0; w < NW; ++w) bad |= wbad[w][lane] != 0;
            if constexpr (kGen) bad |= ((mdead >> lane) & 1u) != 0;
            if (!bad) {   // (a cons3 failure's vp is +inf: no chain to fold)
                // batches of 2 kB terms (pair reads), the next batch's reads in flight while this
                // batch's adds run; ping-pong buffers, the reads past the last batch re-read it
                // (clamped) and are never added
                constexpr int kB = 6;
                const double2* row2 = reinterpret_cast<const double2*>(&term[lane][0]);
                const int nfull = N / (2 * kB);
                __builtin_amdgcn_s_setprio(3);   // the launch's critical path: first at issue
                auto batch = [&](double2 (&buf)[kB], int bt) {
                    const int at = (bt < nfull ? bt : nfull - 1) * kB;
#pragma unroll
                    for (int j = 0; j < kB; ++j) buf[j] = row2[at + j];
                };
                auto add = [&](const double2 (&buf)[kB]) {
#pragma unroll
                    for (int j = 0; j < kB; ++j) {
                        acc += buf[j].x;
                        acc += buf[j].y;
                    }
                };
                if (nfull > 0) {
                    double2 A[kB], B[kB];
                    batch(A, 0);
#pragma unroll 1
                    for (int bt = 0; bt < nfull; bt += 2) {
                        batch(B, bt + 1);
                        __builtin_amdgcn_sched_barrier(0);   // (the reads stay ahead of the adds)
                        add(A);
                        if (bt + 1 >= nfull) break;
                        batch(A, bt + 2);
                        __builtin_amdgcn_sched_barrier(0);
                        add(B);
                    }
                }
                for (int q = nfull * 2 * kB; q < N; ++q) acc += term[lane][q];
                __builtin_amdgcn_s_setprio(0);
            }
            MAC_PREP_STAMP_T(3, kPrepU);
            if (cand(lane) < K) {
                a.vp[cand(lane)] = bad ? __builtin_inf() : acc * a.penalty;
                if (a.dead8) a.dead8[cand(lane)] = excl && bad ? 1 : 0;
            }
        }
        if (obj && a.feas) {   // the evaluations: candidates that pass cons3
            const uint64_t ok = __ballot(lane < NC && cand(lane) < K && !bad);
            if (lane == 0 && ok) atomicAdd(a.feas, (unsigned long long)__popcll(ok));
        }
    } else {
        // per candidate slot its key word (escapes: the fp32 offsets, k_index.h "Keys") and its
        // share of the displacement bound (k_fiw.h sup_box: live candidates only — r > 0, a finite
        // centre, not a cons3 failure; a NaN difference counts as +inf)
        double dmx = -__builtin_inf(), dmy = -__builtin_inf(), dmr = -__builtin_inf(), dml = -__builtin_inf();
        // (matrix) the packed slots' share of the bound, as integers: a key that packs has proved
        // v - base == (double)d bit for bit (key_int), so |x - x0|, |y - y0|, r - r0 and r0 - r are
        // (double)|dx|, (double)|dy|, (double)dr and -(double)dr exactly (IEEE subtraction is
        // antisymmetric), and the maximum is the same in either type. INT_MIN: none yet.
        [[maybe_unused]] int mix = INT_MIN, miy = INT_MIN, mir = INT_MIN, mil = INT_MIN;
        uint32_t pk[NC];
        bool kb = false;   // (records) a key of this disk is inexact (k_index.h "Keys")
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if constexpr (!kGen) {
                if (c == PC && !has7) {   // an absent slot: no key, no share of the bound
                    pk[c] = kKeyEsc;
                    continue;
                }
            }
            const double x = v[c][0], y = v[c][1], r = v[c][2];
            int dx = 0, dy = 0, dr = 0;
            bool packs;
            if constexpr (kMesh == kMeshKeys) {   // (stored above; no fp32 row: an escape is the identity map)
                packs = !((mkbad >> c) & 1u);
                pk[c] = 0u;
                kb |= !packs && !((dead >> c) & 1u);
            } else {
                packs = key_int(x, base[0], 1023.0, dx) && key_int(y, base[1], 1023.0, dy) &&
                        key_int(r, base[2], 511.0, dr);
                pk[c] = packs ? key_pack(dx, dy, dr) : kKeyEsc;
            }
            if (kMesh != kMeshKeys && !packs && iv && cand(c) < K) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const float f = (float)(v[c][q] - base[q]);
                    if constexpr (kGen)
                        kb |= !((dead >> c) & 1u) &&
                              __builtin_bit_cast(uint64_t, base[q] + (double)f) != __builtin_bit_cast(uint64_t, v[c][q]);
                    a.keysT[(int64_t)(q * N + u) * a.ldk + cand(c)] = f;
                }
            }
            if constexpr (kGen) {
                if (a.pd && iv && cand(c) < K && !((dead >> c) & 1u) && r > 0.0 && __builtin_isfinite(x) &&
                    __builtin_isfinite(y)) {
                    double ex = __builtin_fabs(x - base[0]), ey = __builtin_fabs(y - base[1]), er = r - base[2];
                    double el = base[2] - r;
                    if (!(ex <= kDblMax)) ex = __builtin_inf();
                    if (!(ey <= kDblMax)) ey = __builtin_inf();
                    if (!(er == er)) er = __builtin_inf();
                    if (!(el == el)) el = __builtin_inf();
                    dmx = fmax(dmx, ex);
                    dmy = fmax(dmy, ey);
                    dmr = fmax(dmr, er);
                    dml = fmax(dml, el);
                }
            } else {
                // (a packed x or y is finite: its offset from the base is a finite double)
                const bool live = a.pd && iv && cand(c) < K && !((dead >> c) & 1u) && r > 0.0;
                if (live && packs) {
                    mix = max(mix, abs(dx));
                    miy = max(miy, abs(dy));
                    mir = max(mir, dr);
                    mil = max(mil, -dr);
                }
                // an escaped live slot: today's fp64 code; a wave without one executes none of it
                const bool esc = live && !packs;
                if (__ballot(esc) != 0) {
                    if (esc && __builtin_isfinite(x) && __builtin_isfinite(y)) {   // (the generated builds' code above)
                        double ex = __builtin_fabs(x - base[0]), ey = __builtin_fabs(y - base[1]), er = r - base[2];
                        double el = base[2] - r;
                        if (!(ex <= kDblMax)) ex = __builtin_inf();
                        if (!(ey <= kDblMax)) ey = __builtin_inf();
                        if (!(er == er)) er = __builtin_inf();
                        if (!(el == el)) el = __builtin_inf();
                        dmx = fmax(dmx, ex);
                        dmy = fmax(dmy, ey);
                        dmr = fmax(dmr, er);
                        dml = fmax(dml, el);
                    }
                }
            }
        }
        if constexpr (!kGen) {
            if (a.pd) {
                dmx = fmax(dmx, mix == INT_MIN ? -__builtin_inf() : (double)mix);
                dmy = fmax(dmy, miy == INT_MIN ? -__builtin_inf() : (double)miy);
                dmr = fmax(dmr, mir == INT_MIN ? -__builtin_inf() : (double)mir);
                dml = fmax(dml, mil == INT_MIN ? -__builtin_inf() : (double)mil);
            }
        }
        if (kMesh != kMeshKeys && iv) {
            uint32_t* const krow = a.keysP + (int64_t)u * a.ldk;
            if constexpr (kGen) {   // two runs of three words (plus and minus candidates)
#pragma unroll
                for (int c = 0; c < NC; ++c) krow[cand(c)] = pk[c];
            } else {   // (k0 = PC * cw: even) 8-B stores, the extra word alone
                static_assert(PC % 2 == 0, "an even candidate count");
#pragma unroll
                for (int h = 0; h < PC / 2; ++h)
                    *reinterpret_cast<uint2*>(krow + k0 + 2 * h) = make_uint2(pk[2 * h], pk[2 * h + 1]);
                if (has7) krow[cand(PC)] = pk[PC];
            }
        }
        if (kGen && a.prec && iv) {
            // (generated polls only: a matrix source takes this kernel in the fused chain alone)
            // the five-launch chain's partial region record (prep_block's): a tile box holding the
            // spans of the live candidates' disks, the span-area estimate and the key flag
            double xa = __builtin_inf(), xb = -__builtin_inf(), ya = __builtin_inf(), yb = -__builtin_inf();
            double xm = 0.0, ym = 0.0, est = 0.0;
            bool any = false;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const double x = v[c][0], y = v[c][1], r = v[c][2];
                if (cand(c) < K && !((dead >> c) & 1u) && r > 0.0 && __builtin_isfinite(x) &&
                    __builtin_isfinite(y)) {
                    any = true;
                    xa = fmin(xa, x - r);
                    xb = fmax(xb, x + r);
                    ya = fmin(ya, y - r);
                    yb = fmax(yb, y + r);
                    xm = fmax(xm, __builtin_fabs(x) + r);
                    ym = fmax(ym, __builtin_fabs(y) + r);
                    const double e = 2.0 * r * a.g.invS + 1.0;
                    est += e * e;
                }
            }
            int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
            any = any && partial_range(xa, xb, xm, a.g.gx0, a.g.invS, a.g.nTx, x0, x1) &&
                  partial_range(ya, yb, ym, a.g.gy0, a.g.invS, a.g.nTy, y0, y1);
            a.prec[(int64_t)cw * N + u] =
                make_int4((int)range_pack(any, x0, x1, range_shift(a.g.nTx)),
                          (int)range_pack(any, y0, y1, range_shift(a.g.nTy)),
                          __builtin_bit_cast(int, (float)est), kb ? 1 : 0);
        }
        if (a.pd) {
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                dmx = fmax(dmx, __shfl_xor(dmx, o, kWave));
                dmy = fmax(dmy, __shfl_xor(dmy, o, kWave));
                dmr = fmax(dmr, __shfl_xor(dmr, o, kWave));
                dml = fmax(dml, __shfl_xor(dml, o, kWave));
            }
            if (lane == 0) {
                dred[wid][0] = dmx;
                dred[wid][1] = dmy;
                dred[wid][2] = dmr;
                dred[wid][3] = dml;
            }
        }
        MAC_PREP_STAMP(4);   // (diagnostic) wave 0 at the end of its keys and bound
    }
    if (a.pd) {   // the workgroup's displacement bound: the waves' shares in order
        lds_barrier();
        if (u == 0) {
            double4 m = make_double4(dred[0][0], dred[0][1], dred[0][2], dred[0][3]);
            for (int q = 1; q < NW; ++q) {
                m.x = fmax(m.x, dred[q][0]);
                m.y = fmax(m.y, dred[q][1]);
                m.z = fmax(m.z, dred[q][2]);
                m.w = fmax(m.w, dred[q][3]);
            }
            a.pd[cw] = m;
        }
    }
}

template <int PC, bool kX = false, bool kGen = false, int kMesh = 0>
__device__ __forceinline__ void prep_body(uint64_t* ts, PrepArgs& a)
{
    ts_begin(ts);   // profiling only (the chain's first launch: k_common.h)
    if (a.lreset && blockIdx.x == 0 && threadIdx.x == 0) *a.lreset = 0;   // (read by fin2 after fiw)
    if (!a.src.resolve(true)) {
        ts_end(ts);
        return;
    }
    // XCD-aware: workgroups b and b + 8 share an XCD (round-robin dispatch), so consecutive
    // candidate groups — which fill the same lines of keysP and of the records — go to one XCD
    const int per = (int)((gridDim.x + 7) / 8), b = (int)blockIdx.x;
    const int cw = (int)(gridDim.x % 8) == 0 ? (b % 8) * per + b / 8 : b;
    __shared__ __attribute__((aligned(16))) unsigned char lds[sizeof(PrepLds<kX ? PC + 1 : PC>)];
    if constexpr (kX) {   // (N <= kPrepU) a matrix, or a generated complete poll in column triples
        prep_block_x<kGen, kMesh>(a, cw, lds);
    } else if (!kMesh && a.src.cands) {
        prep_block<true, PC>(a, cw, lds);
    } else {
        prep_block<false, PC, kMesh>(a, cw, lds);
    }
    ts_end(ts);
}

// kPrepC candidates per workgroup, two workgroups per CU
// kMesh: a generated poll on a mesh (mac_mads_mesh), its own build: without a mesh the code it was
template <int kMesh = 0>
__global__ __launch_bounds__(kPrepU) __attribute__((amdgpu_waves_per_eu(4))) void prep_kernel(uint64_t* ts, PrepArgs a)
{
    prep_body<kPrepC, false, false, kMesh>(ts, a);
}

// the fused chain's prep over a matrix source: kPrepCX (+1) candidates per workgroup (xbase), a
// ninth wave folding the chains; two workgroups (18 waves) per CU. kGen: a generated complete poll
// in column triples, its own kernel: one code path per register allocation (80 VGPRs each; the
// matrix path spill-free, where one kernel holding both paths spilled 13 VGPRs: config 4's prep
// 20.7 -> 26.1 us). 6 waves per EU beat 5 for the generated path too (prep 17.9 vs 23.7 us with
// 82 VGPRs and no spill: the two it spills here are off the hot path)
template <bool kGen, int kMesh = 0>   // (kMesh: as prep_kernel's; generated polls only)
__global__ __launch_bounds__(kPrepU + kWave) __attribute__((amdgpu_waves_per_eu(6))) void prep_x_kernel(uint64_t* ts, PrepArgs a)
{
    static_assert(kGen || !kMesh, "a mesh belongs to a generated poll");
    prep_body<kPrepCX, true, kGen, kMesh>(ts, a);
}

// cands: see CandSrc. Writes disks[k*N + i] (the streaming scan's records).
__global__ void disk_prep_kernel(CandSrc src, int N, int K, DiskRec* __restrict__ disks)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)N * K) return;
    const int k = (int)(t / N), i = (int)(t % N);
    disks[t] = make_disk(src.get(k, i, N), src.get(k, N + i, N), src.get(k, 2 * N + i, N));
}

}  // namespace mac
