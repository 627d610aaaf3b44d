// eval_plan.h — host only: the request enqueue_eval takes (EvalReq) and the route it takes for it
// (EvalPlan, eval_plan). The plan is every decision that follows from the request's shape and the
// context's options alone: no lane, no device, no launch and no routing history (the histories
// are read where the chains are chosen and sized, maxcover.hip enqueue_eval). mac_diag_route exports
// it for the CPU tests (tests/test_shape_edges.py). Included by maxcover.hip after kernels.h and its
// own routing constants (kPollMinK, kTiledMaxN).
#pragma once

#include <algorithm>
#include <cstdint>

// prog_h_kernel's launch inside a generated poll (k_prog.h; mac_mads_run_prog)
struct ProgLaunch {
    mac::ProgArgs a;
    double h_max;
    double* d_h;   // K doubles
};

// One evaluation: K candidates of N disks from `src`, on the stream enqueue_eval is given. All
// pointers device. The outputs may be null (d_best: no argmin).
struct EvalReq {
    mac::CandSrc src{};
    int N = 0, K = 0;
    bool tiled = false;                    // the tiled family (use_tiled), else the streaming scan
    // the objective's penalty and cons3. d_dlimT: cons3 thresholds per UAV (host calls), else
    // d_dlim_raw: the raw d_lim, thresholded where it is read (device calls)
    const double* d_rmax = nullptr;
    double penalty = 0.0;
    const double* d_prev = nullptr;
    const double* d_dlimT = nullptr;
    const double* d_dlim_raw = nullptr;
    double tan_half_fov = 0.0;
    double* d_area = nullptr;
    double* d_obj = nullptr;
    double* d_best = nullptr;
    int64_t idx_base = 0;
    // the argmin's mapped result slot (k_final.h mirror_check)
    uint64_t* d_mirror = nullptr;
    uint64_t mirror_seq = 0;
    // the native MADS driver: the pipelined loop's update fields and feasible counter, and a
    // generated poll's swarm mask, motion constraints and progressive-barrier launch
    const mac::FinBest* fb_mads = nullptr;
    unsigned long long* d_feas = nullptr;
    const mac::ConsArgs* cons = nullptr;
    const mac::MotionArgs* motion = nullptr;
    const ProgLaunch* prog = nullptr;
    // ... and its verdicts (MAC_OPT_VERDICTS; k_cons.h cons_explain_gen_kernel): the constraints that are
    // on and the context's tally; one more launch behind the prep, read by nothing of the chain
    const mac::ExplainArgs* explain = nullptr;
    unsigned long long* d_tally = nullptr;
};

// What eval_plan reads: the context's options and list facts, the source's kind, the outputs wanted.
struct RouteIn {
    int algo = MAC_ALGO_AUTO, chain = MAC_CHAIN_AUTO, cus = 256;
    int64_t M = 0;
    bool w_uniform = false;
    enum Kind { kMatrix = 0, kBasis = 1, kGenerated = 2 };   // cands / ltri / the stream's draws
    int kind = kMatrix;
    int np = 0, k0 = 0;                    // (generated and basis-form sources: CandSrc.np, k0)
    bool mesh = false, mst = false, route_five = false;
    bool mesh_keys = false;                // MAC_OPT_MESH_KEYS (with a mesh: the kMeshKeys builds)
    int64_t b = 0;
    double delta = 0.0;
    bool want_area = false, want_obj = false;
    bool cons3 = false, mask = false;      // d_prev given; a feasibility byte per candidate
    bool tiled = false;
    int N = 0, K = 0;
};

enum PrepKind { kPrepChains = 0, kPrepXMatrix = 1, kPrepXGen = 2 };   // prep_kernel, prep_x_kernel<false>, <true>

struct EvalPlan {
    bool poll_possible;    // the poll walk's chain runs (else the scan or the per-candidate walk alone)
    int walk_forced;       // kModePoll / kModeTiled, 0: the device's choice (k_poll_shared.h walk_choice)
    int iper;              // candidates per index thread: 3 (K <= 3073), 6 (K <= 6145); 0: identity map
    bool want_keys;        // the index hashes the prep's packed keys
    bool pair, gen_x;      // generated complete polls: the prep's layouts (k_prep.h)
    int mesh;              // a generated poll on a mesh: the chains' kMesh builds (1 value keys, 2 mesh keys)
    int nchain;            // prep_kernel's workgroups
    int G;                 // the per-candidate walk's slices per candidate
    int64_t units;         // ... and its (candidate, slice) units
    bool fused_eligible;   // the fused chain may run; AUTO's history decides (enqueue_eval)
    bool excl;             // cons3 / mask failures are left out of the walk
    int counts;            // equal weights: integer count rows
    int prep_fused, nprep, xbase;   // the fused chain's prep launch
    bool prep_five_runs;            // the five-launch chain's (also without a chain: the penalties)
    int prep_five, nrec;
    unsigned nfw, nidx;    // fiw_kernel's, disk_index_kernel's workgroups
    unsigned nfin2, nfin;  // fin2_kernel's, finalize_kernel's
};

// The poll walk's chain (prep keys and records, disk index, walk choice, poll kernel) runs for an
// evaluation: the tiled family, candidates and entries present, and the poll walk allowed.
static inline bool poll_walk_possible(int algo, int64_t M, int N, int K, bool tiled)
{
    return tiled && N > 0 && M > 0 &&
           (algo == MAC_ALGO_POLL || N > kTiledMaxN ||
            ((algo == MAC_ALGO_AUTO || algo == MAC_ALGO_TILED) && K >= kPollMinK));
}

static inline EvalPlan eval_plan(const RouteIn& in)
{
    using namespace mac;
    const int N = in.N, K = in.K;
    const bool gen = in.kind != RouteIn::kMatrix;
    EvalPlan p{};
    const bool big = N > kTiledMaxN;
    // the poll chain's walk: forced by the algorithm option (or N past the per-candidate walk's
    // LDS limit)
    p.walk_forced = (in.algo == MAC_ALGO_POLL || big) ? kModePoll : in.algo == MAC_ALGO_TILED ? kModeTiled : 0;
    p.poll_possible = poll_walk_possible(in.algo, in.M, N, K, in.tiled);
    p.iper = K <= kIndexMaxK + 1 ? kIdxPer : K <= kIndexMaxKWide + 1 ? kIdxPerWide : 0;
    p.want_keys = p.poll_possible && p.iper;
    p.mesh = gen && in.mesh ? (in.mesh_keys && in.kind == RouteIn::kGenerated ? mac::kMeshKeys : 1) : 0;
    const int target = 8 * in.cus;
    p.G = (int)std::max<int64_t>(1, std::min<int64_t>((target + K - 1) / K, std::max(1, N / kWavesPerBlock)));
    p.units = (int64_t)K * p.G;
    // generated complete polls (the native MADS loop: K = 2n): the prep draws each B entry once
    // for its plus and minus candidates (k_prep.h PrepArgs.pair)
    // (n = the polled variables: 3N, or 2N for an xy-only poll)
    const int npoll = in.np ? in.np : 3 * N;
    p.pair = gen && in.k0 == 0 && K == 2 * npoll && npoll % 4 == 0 && kPrepC == 8;
    // ... or, with one block of UAVs, prep_x_kernel's layout (k_prep.h prep_block_x<true>): a column
    // triple of B per workgroup (its plus and minus candidates: 6), N workgroups, a ninth wave
    // folding the penalty chains beside the keys and the records
    // (full polls only: an xy-only poll takes prep_kernel)
    p.gen_x = gen && !in.np && in.k0 == 0 && K == 6 * N && N >= 1 && N <= kPrepU;
    p.nchain = p.pair ? npoll / 4 : (K + kPrepC - 1) / kPrepC;

    // The fused chain (k_fiw.h: prep -> fiw -> fin2) whenever the poll walk runs on packed keys of at
    // most kFwMaxK + 1 candidates (and, under AUTO, the context's history allows: enqueue_eval).
    // A generated poll whose step the host knows (a stepper's, not the pipelined loop's) at
    // 2^ell > 8 goes to the five-launch chain under AUTO: its disks spread over more than the
    // index's direct-mapped box (ell <= 3) and its superset boxes overlap widely (config 5's first
    // poll of an MPC step: 0.5 ms fused against ~0.11 ms).
    const bool wide_gen = gen && !in.mst &&
                          (in.kind == RouteIn::kBasis ? (double)in.b * __builtin_fabs(in.delta) > 8.0 : in.b > 8);
    p.fused_eligible = p.poll_possible && p.want_keys && N > 0 && in.M > 0 && K > 0 && K <= kFwMaxK + 1 &&
                       in.chain != MAC_CHAIN_FIVE && p.walk_forced != kModeTiled &&
                       (in.chain == MAC_CHAIN_FUSED || (!wide_gen && !in.route_five));
    // cons3 failures are left out of the walk when only objectives are asked for
    p.excl = in.want_obj && (in.cons3 || in.mask) && !in.want_area && N <= kPrepU;
    p.counts = p.poll_possible && in.w_uniform ? 1 : 0;   // equal weights: the walks count

    // the fused chain's prep. A matrix source: kPrepCX (+1) candidates per workgroup (k_prep.h
    // prep_x_kernel)
    const int gx = K / kPrepCX;
    const bool xk = !gen && N <= kPrepU && gx >= 1 && K - gx * kPrepCX <= gx;
    p.prep_fused = p.gen_x ? kPrepXGen : xk ? kPrepXMatrix : kPrepChains;
    p.nprep = p.gen_x ? N : xk ? gx : p.nchain;
    p.xbase = gx * kPrepCX;
    // the five-launch chain's: penalty chains + cons3, the poll walk's partial regions and the
    // index's keys; a generated complete poll with the index's keys in prep_x_kernel's layout
    p.prep_five_runs = (in.want_obj || p.poll_possible) && K > 0;
    p.prep_five = p.gen_x && p.want_keys ? kPrepXGen : kPrepChains;
    p.nrec = p.prep_five == kPrepXGen ? N : p.nchain;

    p.nfw = p.nidx = 8 * (unsigned)((N + 7) / 8);   // one per XCD and disk group
    p.nfin2 = 8 * (unsigned)((K + 8 * kF2C - 1) / (8 * kF2C));
    p.nfin = 8 * (unsigned)((K + 8 * kFinC - 1) / (8 * kFinC));   // k_final.h: XCD map
    return p;
}
