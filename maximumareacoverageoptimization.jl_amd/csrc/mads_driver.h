// mads_driver.h — host only: the native MADS driver (mac_mads_begin* / _poll / _update / _poll_ahead /
// _advance / _result, the pipelined mac_mads_run*, the progressive barrier's mac_mads_run_prog and its
// stepper mac_mads_begin_prog / _poll_prog / _advance_prog / _result_prog with mac_prog_merge) on
// mads_walk.h's arithmetic. Included once by maxcover.hip, after everything the driver calls
// (enqueue_eval, the lanes, the constraint uploads, prog_select_launch, prog_part_launch).
#pragma once

#include "mads_walk.h"

extern "C" {

// The native MADS loop as a stepper (mac_mads_begin / _poll / _update / _result): one
// iteration = one complete LTMADS poll generated on the device. A stepper may own a shard
// [lo, hi) of every poll's 2n candidates: the ranks of a multi-GPU run poll their shards, combine
// their local bests (16 B each, lexicographic (objective, index) minimum) and all apply the same
// update, so they stay in lock step with the single-GPU loop (mac_mads_run = one stepper owning
// the whole poll).
struct MadsProg;   // the progressive barrier's state of a prog stepper (mac_mads_begin_prog, below)
struct mac_mads {
    mac_ctx* ctx = nullptr;
    Lane* L = nullptr;
    hipStream_t s = nullptr;
    int N = 0, n = 0, K = 0;
    int np = 0;                   // polled variables (the basis's size): n, or 2N under MAC_POLL_XY; K = 2 np
    bool xy = false;              // MAC_POLL_XY: x[np..n), the radii, stay as they are
    int64_t lo = 0, hi = 0;
    mac_mads_params prm{};
    double penalty = 1e5, tan_half_fov = 1.0;
    const double* d_prev = nullptr;
    const double* d_dlimT = nullptr;
    ConsArgs cons{};              // the swarm constraints (mac_mads_begin_cons): every poll's mask launch
    bool has_cons = false;
    MotionArgs mot{};             // the motion constraints (mac_mads_begin_motion): the mask launch's tests;
    bool has_mot = false;         // has_cons is set with them (the arrays: the lane's motion buffer)
    std::vector<double> x;
    double f = INFINITY;
    int64_t evals = 0, it = 0, rejected = 0, succ = 0;
    int ell = 0;
    std::vector<double> h_prev;   // cons3's prev (host copy: whole-poll rejection, poll_rejected)
    DevBuf d_feas;                // candidates that passed cons3 (the prep launches count them)
    uint64_t feas_seen = 0;       // d_feas as the last mac_mads_poll_ahead read it
    MadsStream stream;            // the run's draws (mads_walk.h): state = the current iteration's
    std::vector<int> rp, cp, rp_next, cp_next;
    double* hb = nullptr;
    double* hx = nullptr;
    // the poll's best, written by finalize's last block into a mapped slot {obj bits, index,
    // seq, check} (k_final.h): read here without a copy or a stream synchronisation
    PinnedBuf hslot;
    uint64_t* d_slot = nullptr;
    uint64_t seq = 0;
    bool slotted = false;
    int64_t slot_fallbacks = 0;   // slot waits that timed out (copy + sync instead)
    int route_five = 0;           // the polls are crowded (host_crowded_disks at begin): five-launch chain
    int mesh_keys = 0;            // the run keys its polls in mesh units (MAC_OPT_MESH_KEYS as it began, on a mesh)
    // verdicts (MAC_OPT_VERDICTS as the stepper began, with cons3 or a swarm or motion constraint on, no
    // mac_prog): every generated poll's explain launch (k_cons.h) and the context's tally it adds to
    ExplainArgs explain{};
    unsigned long long* d_tally = nullptr;   // null: off
    double* ext_best = nullptr;   // mac_mads_best_buffer: the polls' best goes here
    // the mesh (mac_mads_begin_mesh): the granularity of every variable, host copy and device copy
    // (empty / null: 1.0 everywhere, the calls without a mesh)
    std::vector<double> g;
    DevBuf d_gran;
    const double* d_g = nullptr;
    int64_t polled_b = 0;        // 2^ell of the poll awaiting its update (0: none)
    double h_enq = 0, h_perm = 0, h_wait = 0, h_post = 0;
    std::chrono::steady_clock::time_point t0;
    // the pipelined loop (mads_run_pipelined): incumbent double buffer, device state, permutation
    // rings
    DevBuf d_x, d_st, d_ring;
    PinnedBuf h_ring;
    MadsProg* pg = nullptr;       // a prog stepper: stepped by mac_mads_poll_prog / _advance_prog alone
    ~mac_mads();
};

// An incumbent of the progressive barrier: F (h == 0) or I (0 < h <= h_max).
struct ProgInc {
    std::vector<double> x;
    double f = INFINITY, h = 0.0;
    bool has = false;
};

struct MadsProg {
    ProgArgs pargs{};
    ProgInc F, I;
    double h_max = INFINITY;
    int64_t n_dom = 0, n_imp = 0, n_uns = 0, two = 0, evaluated = 0;
    // pinned staging: per centre [centre 8n][permutations 4*2np][h fill 8 Kc], then the record
    PinnedBuf stage;
    size_t stage_c = 0, stage_sz = 0;
    ProgPart* h_part = nullptr;
    char* d_xinc[2] = {nullptr, nullptr};
    double* d_h[2] = {nullptr, nullptr};
    ProgScalars scalars() const { return ProgScalars{F.has, I.has, F.f, I.f, I.h, h_max}; }
    ~MadsProg() { stage.release(); }
};

inline mac_mads::~mac_mads()
{
    delete pg;
    d_x.release();
    d_gran.release();
    d_feas.release();
    d_st.release();
    d_ring.release();
    h_ring.release();
}

static double* mads_best_ptr(mac_mads* m) { return m->ext_best ? m->ext_best : m->L->best.as<double>(); }

using MadsClock = std::chrono::steady_clock;
static double mads_secs(MadsClock::time_point a, MadsClock::time_point b)
{
    return std::chrono::duration<double>(b - a).count();
}

// every candidate of a whole poll: 2 n_p (n_p = 3N, or 2N for the xy-only poll)
static int64_t mads_poll_count(int64_t three_n, bool xy) { return xy ? 4 * (three_n / 3) : 2 * three_n; }

// the poll of the current iteration at mesh step b with the permutations (rp, cp), as mads_walk.h takes it
static MadsPoll mads_poll_at(const mac_mads* m, int64_t b, const std::vector<int>& rp, const std::vector<int>& cp)
{
    return MadsPoll{m->stream.state, m->np, b, rp.data(), cp.data(), m->g.empty() ? nullptr : m->g.data()};
}

// The generated source of a poll of m's run at (state, b): the centre in the device block d_xinc (3N
// doubles), the permutations at d_perm (rp, then cp: n_p ints each), this source's first candidate k0 of
// the poll; mst: the pipelined loop's device state (b from there).
static CandSrc mads_gen_src(const mac_mads* m, const double* d_xinc, const int* d_perm, uint64_t state, int64_t b,
                            int k0, const MadsState* mst = nullptr)
{
    CandSrc src{};
    src.xinc = d_xinc;
    src.rp = d_perm;
    src.cp = d_perm + m->np;
    src.np = m->xy ? m->np : 0;
    src.state = state;
    src.b = b;
    src.k0 = k0;
    src.mst = mst;
    src.route_five = m->route_five;
    src.set_mesh(m->d_g);
    src.mesh_keys = m->mesh_keys;
    return src;
}

// A centre x and the permutations (rp, cp) into the pinned block h as [centre 8n][rp 4 n_p][cp 4 n_p]
// (n = 3N), and its one copy to the device block d. Returns the device's permutations.
static const int* mads_stage(mac_mads* m, const double* x, const std::vector<int>& rp, const std::vector<int>& cp,
                             void* h, void* d)
{
    const int n = m->n, np = m->np;
    double* hx = static_cast<double*>(h);
    int* hperm = reinterpret_cast<int*>(hx + n);
    std::copy(x, x + n, hx);
    std::copy(rp.begin(), rp.end(), hperm);
    std::copy(cp.begin(), cp.end(), hperm + np);
    HCK(hipMemcpyAsync(d, h, sizeof(double) * n + sizeof(int) * 2 * np, hipMemcpyHostToDevice, m->s));
    return reinterpret_cast<const int*>(static_cast<const double*>(d) + n);
}

// Whether cons3 rejects every candidate of the poll at mesh step b around x (k_prep.h
// diag_rejects for each of the 3N variables: each is the diagonal of one column of B, so each
// candidate carries one such step). Exact: the prep's cons3 would mark every candidate failed,
// and the poll's result would be (+inf, -1).
// (x: the poll's centre; null: the stepper's incumbent)
static bool poll_rejected(const mac_mads* m, int64_t b, const double* x = nullptr)
{
    if (!m->d_prev) return false;
    if (!x) x = m->x.data();
    const int N = m->N;
    const std::vector<double>& T3 = m->L->h_dlim;
    for (int v = 0; v < m->np; ++v) {   // (the polled variables; on a mesh v's step is g[v] * b)
        const int q = v / N, i = v % N;
        const double bv = m->g.empty() ? (double)b : m->g[v] * (double)b;
        if (!diag_rejects(x[v], bv, m->h_prev[v], q, m->tan_half_fov, T3[i])) return false;
    }
    return true;
}

// slot: the poll's best through the mapped slot finalize's last block writes (mads_wait_best),
// else a 16-B copy
static void mads_make_slot(mac_mads* m)
{
    if (m->d_slot) return;
    m->hslot.reserve(64, hipHostMallocMapped | hipHostMallocCoherent);
    std::memset(m->hslot.p, 0, 64);
    void* dp = nullptr;
    HCK(hipHostGetDevicePointer(&dp, m->hslot.p, 0));
    m->d_slot = (uint64_t*)dp;
}

// A stepper's poll of Kc candidates from src as a request: its penalty and cons3 inputs, the lane's
// objectives, the poll's best, and the swarm and motion constraints that are on.
static EvalReq mads_request(mac_mads* m, const CandSrc& src, int Kc)
{
    EvalReq rq;
    rq.src = src;
    rq.N = m->N;
    rq.K = Kc;
    rq.tiled = use_tiled(m->ctx, m->N, nullptr, m->n);
    rq.d_rmax = m->L->rmax.as<double>();
    rq.penalty = m->penalty;
    rq.d_prev = m->d_prev;
    rq.d_dlimT = m->d_dlimT;
    rq.d_dlim_raw = m->d_prev ? m->L->dlimraw.as<double>() : nullptr;
    rq.tan_half_fov = m->tan_half_fov;
    rq.d_obj = m->L->obj.as<double>();
    rq.d_best = mads_best_ptr(m);
    rq.cons = m->has_cons ? &m->cons : nullptr;
    rq.motion = m->has_mot ? &m->mot : nullptr;
    if (m->d_tally) {
        rq.explain = &m->explain;
        rq.d_tally = m->d_tally;
    }
    return rq;
}

static void mads_best_of(mac_mads* m, const CandSrc& src, int Kc, int64_t idx_base, bool slot = false)
{
    if (slot) mads_make_slot(m);
    m->slotted = slot;
    EvalReq rq = mads_request(m, src, Kc);
    rq.idx_base = idx_base;
    if (slot) {
        rq.d_mirror = m->d_slot;
        rq.mirror_seq = ++m->seq;
        rq.d_feas = m->d_feas.as<unsigned long long>();
    }
    enqueue_eval(m->ctx, m->L, m->s, rq);
    if (!slot) HCK(hipMemcpyAsync(m->hb, mads_best_ptr(m), 16, hipMemcpyDeviceToHost, m->s));
}

// The best {objective, global index} of the poll mads_best_of enqueued: from the mapped slot once
// it holds this poll's seq and a matching check word, or, after 50 ms (a failed launch) or
// without a slot, the stream synchronised and the copy.
static void mads_wait_best(mac_mads* m, double* obj, int64_t* idx, uint64_t* feas_cum = nullptr)
{
    if (m->slotted) {
        // a slotted poll always hands finalize the stepper's d_feas (mads_best_of), so the check
        // word folds in the feasible count of word 4: read it whether or not the caller wants it
        // (with f = 0 the check never matched once a candidate had passed cons3, and every wait
        // ran into the 50-ms limit: round 5's sharded-loop stall)
        uint64_t fe = 0;
        if (mirror_wait((const uint64_t*)m->hslot.p, m->seq, 50.0, obj, idx, &fe)) {
            if (feas_cum) *feas_cum = fe;
            return;
        }
        ++m->slot_fallbacks;
        HCK(hipMemcpyAsync(m->hb, mads_best_ptr(m), 16, hipMemcpyDeviceToHost, m->s));
    }
    HCK(hipStreamSynchronize(m->s));
    *obj = m->hb[0];
    *idx = __builtin_bit_cast(int64_t, m->hb[1]);
    if (feas_cum) {
        unsigned long long fe = 0;
        HCK(hipMemcpy(&fe, m->d_feas.p, sizeof(fe), hipMemcpyDeviceToHost));
        *feas_cum = fe;
    }
}

// A poll's explain launch was enqueued with it (mads_request): one tallied launch.
static void mads_count_verdict_poll(mac_mads* m, int64_t polls = 1)
{
    if (m->d_tally && polls > 0) m->ctx->verdict_polls.fetch_add(polls, std::memory_order_relaxed);
}

// The stepper's shard of the poll at (state, b) around its incumbent, with the permutations (rp, cp),
// enqueued through the slot. The lane's staging is free: the previous poll's copy preceded its
// finalize, whose results were read.
static void mads_enqueue_poll(mac_mads* m, uint64_t state, int64_t b, const std::vector<int>& rp,
                              const std::vector<int>& cp)
{
    m->L->xinc.reserve(sizeof(double) * m->n + sizeof(int) * 2 * m->np);
    const int* d_perm = mads_stage(m, m->x.data(), rp, cp, m->hx, m->L->xinc.p);
    mads_best_of(m, mads_gen_src(m, m->L->xinc.as<double>(), d_perm, state, b, (int)m->lo), (int)(m->hi - m->lo),
                 m->lo, true);
    mads_count_verdict_poll(m);
}

static void mads_free(mac_mads* m)
{
    if (!m) return;
    if (m->L) release_lane(m->ctx, m->L, m->s);
    delete m;
}

// The opts of a run or a stepper: MAC_E_INVAL on an unknown poll kind or a non-zero reserved word;
// *xy = the xy-only poll (null opts: the full poll).
static int32_t mads_opts_check(const mac_mads_opts* opts, bool* xy)
{
    *xy = false;
    if (!opts) return MAC_OK;
    if (opts->poll_vars != MAC_POLL_XYR && opts->poll_vars != MAC_POLL_XY)
        return fail(MAC_E_INVAL, "mac_mads_opts: unknown poll_vars " + std::to_string(opts->poll_vars));
    for (int q = 0; q < 3; ++q)
        if (opts->reserved[q] != 0) return fail(MAC_E_INVAL, "mac_mads_opts: reserved must be 0");
    *xy = opts->poll_vars == MAC_POLL_XY;
    return MAC_OK;
}

// The mesh of a run or a stepper: MAC_E_INVAL on a non-zero reserved word or an entry that is not
// finite and > 0, before the context is touched; *gran = the 3N host doubles, or null when the mesh
// is the unit one (no mesh, no vector, or every entry exactly 1.0).
static int32_t mads_mesh_check(const mac_mads_mesh* mesh, int64_t three_n, const double** gran)
{
    *gran = nullptr;
    if (!mesh) return MAC_OK;
    if (mesh->reserved != 0) return fail(MAC_E_INVAL, "mac_mads_mesh: reserved must be 0");
    if (!mesh->granularity) return MAC_OK;
    bool unit = true;
    for (int64_t v = 0; v < three_n; ++v) {
        const double g = mesh->granularity[v];
        if (!(g > 0.0) || !std::isfinite(g))
            return fail(MAC_E_INVAL, "mac_mads_mesh: granularity[" + std::to_string(v) +
                                         "] is not finite and > 0");
        unit = unit && g == 1.0;
    }
    if (!unit) *gran = mesh->granularity;
    return MAC_OK;
}

// What the widest entry points (mac_mads_run_mesh / mac_mads_begin_mesh) take beyond the plain run;
// the narrower ones leave the rest null. mads_setup_check fills xy and gran: the mesh's errors win
// over the opts', and both over every check of the run itself.
struct MadsSetup {
    const mac_cons* cons = nullptr;
    const mac_mads_opts* opts = nullptr;
    const mac_motion* motion = nullptr;   // (every constraint off: as none)
    const mac_mads_mesh* mesh = nullptr;
    bool checked = false, xy = false;
    const double* gran = nullptr;
    bool prog = false;   // a mac_prog run or stepper: MAC_OPT_VERDICTS is ignored (nothing allocated, no check)
    bool verdicts = false;   // MAC_OPT_VERDICTS as the run begins (read once: mads_begin_impl), false under prog
};

static int32_t mads_setup_check(MadsSetup& su, int64_t three_n)
{
    if (su.checked) return MAC_OK;
    int32_t rc = mads_mesh_check(su.mesh, three_n, &su.gran);
    if (!rc) rc = mads_opts_check(su.opts, &su.xy);
    su.checked = !rc;
    return rc;
}

// What a run's arguments come to once they pass its own checks (mads_begin_check).
struct MadsShape {
    int N = 0, n = 0, np = 0, K = 0;   // UAVs, variables 3N, polled variables n_p, a poll's candidates 2 n_p
    ConsArgs ca{};
    bool has_mot = false, has_cons = false;
};

// The run's own checks (after the mesh's and the opts': mads_setup_check), before the device is touched.
static int32_t mads_begin_check(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                                const double* prev, const double* d_lim, const mac_mads_params* prm,
                                int64_t shard_lo, int64_t shard_hi, const MadsSetup& su, MadsShape& sh)
{
    int32_t rc = check_common(ctx, three_n, 1);
    if (rc) return rc;
    if (!x0 || !r_max || !prm) return fail(MAC_E_INVAL, "null argument");
    if (prev && !d_lim) return fail(MAC_E_INVAL, "prev given without d_lim");
    if (prm->ell0 < 0 || prm->ell_max < prm->ell0 || prm->ell_max > 52)
        return fail(MAC_E_INVAL, "need 0 <= ell0 <= ell_max <= 52");
    sh.N = (int)(three_n / 3);
    if (sh.N == 0) return fail(MAC_E_INVAL, "no UAV");
    // np: the polled variables (the basis's size), every poll's candidates K = 2 np
    sh.n = (int)three_n;
    sh.np = su.xy ? 2 * sh.N : sh.n;
    sh.K = (int)mads_poll_count(three_n, su.xy);
    if (shard_lo < 0 || shard_hi > sh.K || shard_lo > shard_hi)
        return fail(MAC_E_INVAL, "shard outside [0, 2n)");
    bool mc, ms, ma;
    sh.has_mot = motion_on(su.motion, &mc, &ms, &ma);
    // (a motion constraint alone: the mask launch with cons7 and cons8 off)
    sh.has_cons = cons_active(su.cons, &sh.ca) | sh.has_mot;
    if (sh.has_cons && sh.N > kConsMaxN)
        return fail(MAC_E_INVAL, "mac_mads_begin_cons: N = " + std::to_string(sh.N) + " > " +
                                     std::to_string(kConsMaxN) + " UAVs under a swarm constraint");
    // the verdict launch sorts as the mask does: with the option on, cons3 alone meets the same limit
    if (su.verdicts && (sh.has_cons || prev) && sh.N > kConsMaxN)
        return fail(MAC_E_INVAL, "MAC_OPT_VERDICTS: N = " + std::to_string(sh.N) + " > " + std::to_string(kConsMaxN) +
                                     " UAVs under a constraint (the verdict kernel's limit)");
    return MAC_OK;
}

// The lane's buffers of a run and its uploads: r_max, the motion constraints (motion null: none on),
// cons3's prev and d_lim, the incumbent x0, the mesh (gran null: none), the pinned staging.
static void mads_begin_buffers(mac_mads* m, const double* x0, const double* r_max, const double* prev,
                               const double* d_lim, const mac_motion* motion, const double* gran)
{
    Lane* L = m->L;
    hipStream_t s = m->s;
    const int N = m->N, n = m->n;
    const int64_t three_n = n;
    L->cands.reserve(sizeof(double) * three_n);
    L->xinc.reserve(sizeof(double) * three_n);
    L->perm.reserve(sizeof(int) * 2 * n);
    L->area.reserve(sizeof(double) * m->K);
    L->obj.reserve(sizeof(double) * m->K);
    L->best.reserve(16);
    L->rmax.reserve(sizeof(double) * N);
    HCK(hipMemcpyAsync(L->rmax.p, r_max, sizeof(double) * N, hipMemcpyHostToDevice, s));
    m->d_feas.reserve(sizeof(unsigned long long));
    HCK(hipMemsetAsync(m->d_feas.p, 0, sizeof(unsigned long long), s));
    if (motion) {
        m->mot = motion_upload(L, s, N, motion);
        m->has_mot = true;
    }
    if (prev) {
        m->h_prev.assign(prev, prev + three_n);
        cons3_upload(L, s, N, prev, d_lim);
        m->d_prev = L->prev.as<double>();
        m->d_dlimT = L->dlim.as<double>();
    }
    m->x.assign(x0, x0 + three_n);
    if (gran) {   // the mesh: validated already (mads_setup_check), copied here
        m->g.assign(gran, gran + three_n);
        m->d_gran.reserve(sizeof(double) * three_n);
        // (pageable memory: the copy has left m->g when the call returns)
        HCK(hipMemcpyAsync(m->d_gran.p, m->g.data(), sizeof(double) * three_n, hipMemcpyHostToDevice, s));
        m->d_g = m->d_gran.as<double>();
    }
    // pinned staging: [best 16 B][incumbent 8*3N][permutations 4*2n]
    L->h_stage.reserve(16 + sizeof(double) * three_n + sizeof(int) * 2 * n);
    m->hb = (double*)L->h_stage.p;
    m->hx = m->hb + 2;
}

// f(x0): the objective, +inf when x0 itself violates cons3 (every rank evaluates it)
static void mads_begin_f0(mac_mads* m)
{
    Lane* L = m->L;
    hipStream_t s = m->s;
    const int N = m->N;
    std::copy(m->x.begin(), m->x.end(), m->hx);
    HCK(hipMemcpyAsync(L->cands.p, m->hx, sizeof(double) * m->n, hipMemcpyHostToDevice, s));
    mads_best_of(m, matrix_src(L->cands.as<double>(), N), 1, 0);
    if (m->has_cons) {   // ... or a swarm constraint: its byte from the matrix mask
        L->cmask.reserve(1);
        cons_mask_enqueue(s, L->cands.as<double>(), N, 1, m->cons, L->cmask.as<uint8_t>(),
                          m->has_mot ? &m->mot : nullptr);
    }
    HCK(hipStreamSynchronize(s));
    m->f = __builtin_bit_cast(int64_t, m->hb[1]) >= 0 ? m->hb[0] : INFINITY;
    if (m->has_cons) {
        uint8_t ok = 1;
        HCK(hipMemcpy(&ok, L->cmask.p, 1, hipMemcpyDeviceToHost));
        if (!ok) m->f = INFINITY;
    }
}

// The run's chain, from its first poll: x0 at mesh step 2^ell0 (the incumbent moves by a few steps over
// a run; crowding is a property of the UAVs' layout).
static void mads_begin_route(mac_mads* m)
{
    const int np = m->np;
    // (on a mesh the largest step, max_v g[v] 2^ell0; a routing estimate only)
    const double gmax = m->g.empty() ? 1.0 : *std::max_element(m->g.begin(), m->g.begin() + np);
    m->route_five = host_crowded_disks(m->x.data(), m->N, gmax * std::ldexp(1.0, m->prm.ell0), m->ctx->grid.S) > kBitsMinDisks ? 1 : 0;
    // A granularity with a non-integer entry: the keys escape to fp32 words or to the identity map
    // (k_prep.h "Packed keys"), which the fused chain walks one position per candidate; the
    // five-launch chain's hash still deduplicates them. Measured at config 5 with g_r = 0.125
    // (tools/mads_granularity_time.py, profiles/mads_granularity.json): 14.6 ms per MPC step
    // through the five-launch chain against 73.9 ms through the fused one. (The polled variables'
    // entries: an xy-only poll never steps by g_r.)
    // With mesh keys (MAC_OPT_MESH_KEYS; mesh_key.h) every granularity packs as the unit mesh does, and
    // AUTO follows the crowding estimate alone. The run keeps the mode it begins with.
    m->mesh_keys = m->ctx->mesh_keys == MAC_KEYS_MESH && !m->g.empty() ? 1 : 0;
    m->route_five = mads_route_five(m->route_five != 0, m->g.empty() ? nullptr : m->g.data(), np, m->mesh_keys != 0);
}

// MAC_OPT_VERDICTS as the run begins (like mesh_keys: the stepper keeps it): with a constraint on, the
// explain launch's arguments from the stepper's own uploads and the context's tally.
static void mads_begin_verdicts(mac_mads* m, bool on)
{
    if (!on || !(m->has_cons || m->d_prev)) return;
    ConsArgs a = m->cons;
    if (!(a.sep || a.zone)) a = cons_args(0.0, NAN, NAN);   // (a motion constraint or cons3 alone)
    m->explain = explain_args(a, m->has_mot ? &m->mot : nullptr, m->d_prev, m->d_dlimT, m->tan_half_fov);
    m->d_tally = verdict_tally(m->ctx);
}

// The stream's seed and the first iteration's permutations. They do not depend on the poll outcomes:
// the next iteration's are computed on the host while the device evaluates the current poll.
static void mads_begin_stream(mac_mads* m)
{
    m->stream = MadsStream{m->prm.seed, m->np};
    m->stream.draw(m->stream.state, m->rp_next, m->cp_next);
}

static int32_t mads_begin_impl(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                               double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                               const mac_mads_params* prm, int64_t shard_lo, int64_t shard_hi,
                               mac_mads** out, MadsSetup su)
{
    ABI_BEGIN
    if (!out) return fail(MAC_E_INVAL, "null out");
    *out = nullptr;
    int32_t rc = mads_setup_check(su, three_n);
    if (rc) return rc;
    // (the option is read once: the size check below and the tally follow the same value)
    su.verdicts = ctx && !su.prog && ctx->verdicts.load(std::memory_order_relaxed) != 0;
    MadsShape sh;
    rc = mads_begin_check(ctx, x0, three_n, r_max, prev, d_lim, prm, shard_lo, shard_hi, su, sh);
    if (rc) return rc;
    set_device(ctx);
    mac_mads* m = new mac_mads();
    m->cons = sh.ca;
    m->has_cons = sh.has_cons;
    m->t0 = MadsClock::now();
    m->ctx = ctx;
    try {
        m->L = acquire_lane(ctx, nullptr);
        m->s = m->L->stream;
        m->N = sh.N;
        m->n = sh.n;
        m->np = sh.np;
        m->xy = su.xy;
        m->K = sh.K;
        m->lo = shard_lo;
        m->hi = shard_hi;
        m->prm = *prm;
        m->penalty = penalty;
        m->tan_half_fov = tan_half_fov;
        mads_begin_buffers(m, x0, r_max, prev, d_lim, sh.has_mot ? su.motion : nullptr, su.gran);
        mads_begin_f0(m);
        m->evals = 1;
        m->ell = prm->ell0;
        mads_begin_route(m);
        mads_begin_stream(m);
        mads_begin_verdicts(m, su.verdicts);
    } catch (...) {
        mads_free(m);
        throw;
    }
    *out = m;
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_poll(mac_mads* m, int32_t* done, double* best_obj, int64_t* best_idx)
{
    ABI_BEGIN
    if (!m || !done || !best_obj || !best_idx) return fail(MAC_E_INVAL, "null argument");
    if (m->pg) return fail(MAC_E_INVAL, "mac_mads_poll on a prog stepper (use mac_mads_poll_prog)");
    if (m->polled_b) return fail(MAC_E_INVAL, "mac_mads_poll twice without mac_mads_update");
    *done = 0;
    if (m->it >= m->prm.n_iter || m->ell < 0) {
        *done = 1;
        return MAC_OK;
    }
    set_device(m->ctx);
    const auto ta = MadsClock::now();
    ++m->it;
    const int64_t b = (int64_t)1 << m->ell;
    m->rp.swap(m->rp_next);
    m->cp.swap(m->cp_next);
    const int Kc = (int)(m->hi - m->lo);
    // a poll cons3 rejects whole: no launch, its result (+inf, -1) (every rank decides alike)
    const bool rejected = Kc > 0 && poll_rejected(m, b);
    if (rejected) {
        ++m->rejected;
        if (m->ext_best) {   // the buffer holds this poll's best once the call returns
            m->hb[0] = INFINITY;
            m->hb[1] = __builtin_bit_cast(double, (int64_t)-1);
            HCK(hipMemcpyAsync(m->ext_best, m->hb, 16, hipMemcpyHostToDevice, m->s));
            HCK(hipStreamSynchronize(m->s));
        }
    }
    if (Kc > 0 && !rejected) mads_enqueue_poll(m, m->stream.state, b, m->rp, m->cp);
    const auto tb = MadsClock::now();
    if (m->it < m->prm.n_iter) m->stream.draw(m->stream.state_after(1), m->rp_next, m->cp_next);
    const auto tc = MadsClock::now();
    if (Kc > 0 && !rejected) {
        mads_wait_best(m, best_obj, best_idx);
    } else {
        *best_obj = INFINITY;
        *best_idx = -1;
    }
    const auto td = MadsClock::now();
    m->polled_b = b;
    m->h_enq += mads_secs(ta, tb);
    m->h_perm += mads_secs(tb, tc);
    m->h_wait += mads_secs(tc, td);
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_update(mac_mads* m, double best_obj, int64_t best_idx)
{
    ABI_BEGIN
    if (!m) return fail(MAC_E_INVAL, "null stepper");
    if (m->pg) return fail(MAC_E_INVAL, "mac_mads_update on a prog stepper (use mac_mads_advance_prog)");
    if (!m->polled_b) return fail(MAC_E_INVAL, "mac_mads_update without a poll");
    if (best_idx >= m->K) return fail(MAC_E_INVAL, "best index outside the poll");
    const auto te0 = MadsClock::now();
    const int64_t b = m->polled_b;
    m->polled_b = 0;
    m->evals += m->K;
    mads_accept(mads_poll_at(m, b, m->rp, m->cp), best_obj, best_idx, (int)m->prm.ell_max, m->x.data(), m->n, m->f,
                m->ell, m->succ);
    m->stream.advance();
    m->h_post += mads_secs(te0, MadsClock::now());
    return MAC_OK;
    ABI_END
}

// Speculation over failure branches (the sharded loop's other mode, dist.mads_loop speculate):
// a failed iteration's next poll is fully determined — the same incumbent, ell - 1 and the next
// stream position — so rank j can evaluate, beside rank 0's real poll, the poll that follows j
// consecutive failures. mac_mads_poll_ahead evaluates it (the whole poll, this stepper's shard)
// without advancing the stepper; mac_mads_advance then applies the gathered results in order, one
// iteration each, up to the first success. Same iterates as the sequential loop.
int32_t mac_mads_poll_ahead(mac_mads* m, int32_t ahead, int32_t* done, double* best_obj, int64_t* best_idx,
                            int64_t* feasible)
{
    ABI_BEGIN
    if (!m || !done || !best_obj || !best_idx) return fail(MAC_E_INVAL, "null argument");
    if (feasible) *feasible = 0;
    if (m->pg) return fail(MAC_E_INVAL, "mac_mads_poll_ahead on a prog stepper (use mac_mads_poll_prog)");
    if (ahead < 0) return fail(MAC_E_INVAL, "negative ahead");
    if (m->polled_b) return fail(MAC_E_INVAL, "mac_mads_poll_ahead with a mac_mads_poll pending");
    *done = 0;
    *best_obj = INFINITY;
    *best_idx = -1;
    if (m->it + ahead >= m->prm.n_iter || m->ell - ahead < 0) {
        *done = 1;
        return MAC_OK;
    }
    set_device(m->ctx);
    const int64_t b = (int64_t)1 << (m->ell - ahead);
    if (m->hi == m->lo) return MAC_OK;
    if (poll_rejected(m, b)) return MAC_OK;   // (counted by mac_mads_advance once applied)
    const uint64_t state = m->stream.state_after((uint64_t)ahead);
    if (ahead == 0) {   // the current iteration's permutations are computed already
        mads_enqueue_poll(m, state, b, m->rp_next, m->cp_next);
    } else {
        std::vector<int> rp, cp;
        m->stream.draw(state, rp, cp);
        mads_enqueue_poll(m, state, b, rp, cp);
    }
    uint64_t fe = 0;
    mads_wait_best(m, best_obj, best_idx, &fe);
    if (feasible) *feasible = (int64_t)(fe - m->feas_seen);
    m->feas_seen = fe;
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_advance(mac_mads* m, double best_obj, int64_t best_idx, int32_t* moved)
{
    ABI_BEGIN
    if (!m) return fail(MAC_E_INVAL, "null stepper");
    if (m->pg) return fail(MAC_E_INVAL, "mac_mads_advance on a prog stepper (use mac_mads_advance_prog)");
    if (m->polled_b) return fail(MAC_E_INVAL, "mac_mads_advance with a mac_mads_poll pending (use mac_mads_update)");
    if (best_idx >= m->K) return fail(MAC_E_INVAL, "best index outside the poll");
    if (m->it >= m->prm.n_iter || m->ell < 0) return fail(MAC_E_INVAL, "mac_mads_advance past the loop's end");
    const int64_t b = (int64_t)1 << m->ell;
    // the applied poll's whole-poll rejection, decided as mac_mads_poll does (the speculating ranks'
    // own polls ahead are not counted: they may never be applied)
    if (m->hi > m->lo && poll_rejected(m, b)) ++m->rejected;
    ++m->it;
    m->evals += m->K;
    // (the current iteration's permutations: rp_next / cp_next)
    const bool better = mads_accept(mads_poll_at(m, b, m->rp_next, m->cp_next), best_obj, best_idx,
                                    (int)m->prm.ell_max, m->x.data(), m->n, m->f, m->ell, m->succ);
    m->stream.advance();
    if (m->it < m->prm.n_iter) m->stream.draw(m->stream.state, m->rp_next, m->cp_next);
    if (moved) *moved = better ? 1 : 0;
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_result(mac_mads* m, double* x_out, mac_mads_stats* st)
{
    ABI_BEGIN
    if (!m) return fail(MAC_E_INVAL, "null stepper");
    if (x_out) std::copy(m->x.begin(), m->x.end(), x_out);
    if (st) {
        st->f = m->f;
        st->iterations = m->it;
        st->evaluations = m->evals;
        st->status = m->ell < 0 ? 0 : 1;
        st->feasible = std::isfinite(m->f) ? 1 : 0;
        st->seconds = mads_secs(m->t0, MadsClock::now());
        st->host_enqueue_s = m->h_enq;
        st->host_perm_s = m->h_perm;
        st->wait_s = m->h_wait;
        st->host_post_s = m->h_post;
        unsigned long long fe = 0;
        set_device(m->ctx);
        HCK(hipMemcpyAsync(&fe, m->d_feas.p, sizeof(fe), hipMemcpyDeviceToHost, m->s));
        HCK(hipStreamSynchronize(m->s));
        st->feasible_evaluations = (int64_t)fe;
        st->rejected_polls = m->rejected;
        st->successes = m->succ;
        st->slot_fallbacks = m->slot_fallbacks;
    }
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_best_buffer(mac_mads* m, void* d_best16)
{
    ABI_BEGIN
    if (!m) return fail(MAC_E_INVAL, "null stepper");
    if (m->pg) return fail(MAC_E_INVAL, "mac_mads_best_buffer on a prog stepper (its polls report a mac_prog_part)");
    if (((uintptr_t)d_best16 & 7) != 0) return fail(MAC_E_INVAL, "d_best16 not 8-byte aligned");
    m->ext_best = (double*)d_best16;
    if (d_best16 && m->hi == m->lo) {   // an empty shard never polls: it offers {+inf, -1}
        set_device(m->ctx);
        const double none[2] = {INFINITY, __builtin_bit_cast(double, (int64_t)-1)};
        HCK(hipMemcpy(d_best16, none, 16, hipMemcpyHostToDevice));
    }
    return MAC_OK;
    ABI_END
}

void mac_mads_destroy(mac_mads* m)
{
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->s);
    mads_free(m);
}

// ------------------------------------------------------------------ pipelined MADS loop
// mac_mads_run on one GPU when the poll walk runs: every poll's finalize applies the poll's update on
// the device (k_final.h mads_step) and the next poll's launches read the mesh index from the device
// state (k_prep.h MadsState), so the host enqueues poll t + kMadsWindow - 1 while poll t runs and
// waits only to bound that window (on the mapped slot's seq word). The permutations do not depend
// on the outcomes: computed kMadsAhead iterations ahead into a pinned ring and uploaded kMadsChunk
// iterations per copy. Same incumbents, objective and counts as the stepper loop, bit for bit (the
// same arithmetic, only where it runs differs): tests/test_gpu_parity.py
// test_native_mads_pipelined_matches_stepper.
static constexpr int kMadsWindow = 3;   // polls in flight
static constexpr int kMadsAhead = 16;   // permutations computed ahead of the enqueued poll
static constexpr int kMadsChunk = 8;    // iterations per permutation upload
static constexpr int kMadsRing = 32;    // permutation slots (device and pinned)
static constexpr uint64_t kMadsDoneSeq = 1ull << 62;   // seq word of a stopped loop

static bool mads_pipelinable(const mac_mads* m)
{
    return m->lo == 0 && m->hi == m->K && !m->ext_best && m->prm.n_iter > 0 &&
           poll_walk_possible(m->ctx->algo, m->ctx->M, m->N, m->K, use_tiled(m->ctx, m->N, nullptr, m->n));
}

static void mads_run_pipelined(mac_mads* m)
{
    const int n = m->n, np = m->np;
    const int64_t n_iter = m->prm.n_iter;
    const size_t slot_ints = 2 * (size_t)np;   // a permutation slot: rp, cp of the polled variables
    hipStream_t s = m->s;
    mads_make_slot(m);
    m->d_x.reserve(sizeof(double) * 2 * n);
    m->d_st.reserve(sizeof(MadsState));
    m->d_ring.reserve(sizeof(int) * slot_ints * kMadsRing);
    m->h_ring.reserve(sizeof(int) * slot_ints * kMadsRing);
    double* dx = m->d_x.as<double>();
    MadsState* dst = m->d_st.as<MadsState>();
    int* dring = m->d_ring.as<int>();
    int* hring = (int*)m->h_ring.p;
    const MadsStream seed = m->stream;   // iteration t's stream state: t - 1 iterations after the seed's
    auto state_of = [&](int64_t t) { return seed.state_after((uint64_t)(t - 1)); };
    auto perms_of = [&](int64_t t) {   // into the pinned ring
        int* h = hring + (size_t)((t - 1) % kMadsRing) * slot_ints;
        seed.draw(state_of(t), m->rp_next, m->cp_next);
        std::memcpy(h, m->rp_next.data(), sizeof(int) * np);
        std::memcpy(h + np, m->cp_next.data(), sizeof(int) * np);
    };
    int64_t uploaded = 0;   // iterations [1, uploaded] on the device
    auto upload_to = [&](int64_t t1) {   // [uploaded + 1, t1]: contiguous slots (chunk aligned)
        const int64_t t0 = uploaded + 1;
        if (t1 < t0) return;
        const size_t q0 = (size_t)((t0 - 1) % kMadsRing);
        HCK(hipMemcpyAsync(dring + q0 * slot_ints, hring + q0 * slot_ints,
                           sizeof(int) * slot_ints * (size_t)(t1 - t0 + 1), hipMemcpyHostToDevice, s));
        uploaded = t1;
    };
    // the incumbent and the state: x0 (begin's pinned staging holds it), f(x0), ell0
    const auto ta = MadsClock::now();
    HCK(hipMemcpyAsync(dx, m->hx, sizeof(double) * n, hipMemcpyHostToDevice, s));
    const MadsState st0{m->f, 0, m->ell, 0, 0ull, 0, 0, m->d_g};
    HCK(hipMemcpy(dst, &st0, sizeof(st0), hipMemcpyHostToDevice));
    int64_t computed = std::min<int64_t>(n_iter, kMadsAhead);
    for (int64_t t = 1; t <= computed; ++t) perms_of(t);
    for (int64_t t = kMadsChunk; t <= computed; t += kMadsChunk) upload_to(t);
    upload_to(computed);
    m->h_perm += mads_secs(ta, MadsClock::now());

    const volatile uint64_t* seqw = (const volatile uint64_t*)m->hslot.p + 2;
    bool stopped = false;
    for (int64_t t = 1; t <= n_iter && !stopped; ++t) {
        const auto t1 = MadsClock::now();
        if (t > kMadsWindow) {   // poll t - kMadsWindow finished (or the loop stopped)
            const uint64_t want = (uint64_t)(t - kMadsWindow);
            for (int spin = 0; *seqw < want; ++spin) {
                if ((spin & 1023) == 1023 &&
                    std::chrono::duration<double, std::milli>(MadsClock::now() - t1).count() > 50.0) {
                    HCK(hipStreamSynchronize(s));   // a failed launch surfaces here
                    if (*seqw < want) throw HipError{hipErrorUnknown, "pipelined MADS poll lost", __LINE__, __FILE_NAME__};
                }
            }
            stopped = *seqw >= kMadsDoneSeq;
            if (stopped) break;
        }
        const auto t2 = MadsClock::now();
        // (b: from the device state)
        const CandSrc src = mads_gen_src(m, dx + (size_t)((t - 1) & 1) * n,
                                         dring + (size_t)((t - 1) % kMadsRing) * slot_ints, state_of(t), 0, 0, dst);
        FinBest fbm{};
        fbm.st = dst;
        fbm.x = src.xinc;
        fbm.x_next = dx + (size_t)(t & 1) * n;
        fbm.rp = src.rp;
        fbm.cp = src.cp;
        fbm.state = src.state;
        fbm.n = n;
        fbm.np = src.np;
        fbm.ell_max = (int)m->prm.ell_max;
        fbm.done_seq = kMadsDoneSeq;
        EvalReq rq = mads_request(m, src, m->K);   // (pipelinable: the tiled family, the lane's best)
        rq.d_mirror = m->d_slot;
        rq.mirror_seq = (uint64_t)t;
        rq.fb_mads = &fbm;
        rq.d_feas = &dst->feas;
        enqueue_eval(m->ctx, m->L, s, rq);
        const auto t3 = MadsClock::now();
        if (computed < n_iter) {   // one iteration's permutations per poll, uploaded per chunk
            perms_of(++computed);
            if (computed % kMadsChunk == 0 || computed == n_iter) upload_to(computed);
        }
        const auto t4 = MadsClock::now();
        m->h_wait += mads_secs(t1, t2);
        m->h_enq += mads_secs(t2, t3);
        m->h_perm += mads_secs(t3, t4);
    }
    const auto t5 = MadsClock::now();
    HCK(hipStreamSynchronize(s));
    MadsState st{};
    HCK(hipMemcpy(&st, dst, sizeof(st), hipMemcpyDeviceToHost));
    HCK(hipMemcpy(m->x.data(), dx + (size_t)(st.it & 1) * n, sizeof(double) * n, hipMemcpyDeviceToHost));
    m->f = st.f;
    m->it = st.it;
    m->ell = st.ell;
    m->evals = 1 + st.it * (int64_t)m->K;
    m->rejected += st.skipped;
    m->succ += st.succ;
    mads_count_verdict_poll(m, st.it - st.skipped);   // (the launches past the stop and of skipped polls returned)
    if (st.feas) {   // (the stepper's counter holds the polls' evaluations: none before this loop)
        const unsigned long long fe = st.feas;
        HCK(hipMemcpy(m->d_feas.p, &fe, sizeof(fe), hipMemcpyHostToDevice));
    }
    m->stream.state = state_of(st.it + 1);
    m->h_wait += mads_secs(t5, MadsClock::now());
}

static int32_t mads_run_impl(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                             double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                             const mac_mads_params* prm, double* x_out, mac_mads_stats* st, MadsSetup su)
{
    ABI_BEGIN
    int32_t rc = mads_setup_check(su, three_n);
    if (rc) return rc;
    if (!x_out) return fail(MAC_E_INVAL, "null argument");
    mac_mads* m = nullptr;
    // the whole poll: every candidate of the 2 n_p (n_p = 3N, or 2N for the xy-only poll)
    rc = mads_begin_impl(ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, 0,
                         mads_poll_count(three_n, su.xy), &m, su);
    if (rc) return rc;
    if (mads_pipelinable(m)) {
        try {
            set_device(ctx);
            mads_run_pipelined(m);
        } catch (...) {
            mac_mads_destroy(m);
            throw;
        }
    } else {
        for (;;) {
            int32_t done = 0;
            double bo = 0.0;
            int64_t bi = -1;
            rc = mac_mads_poll(m, &done, &bo, &bi);
            if (rc || done) break;
            rc = mac_mads_update(m, bo, bi);
            if (rc) break;
        }
    }
    if (!rc) rc = mac_mads_result(m, x_out, st);
    mac_mads_destroy(m);
    return rc;
    ABI_END
}

// The entry points, narrowest first: each is the widest with what it lacks left null.
#define MADS_RUN_ARGS                                                                                      \
    mac_ctx *ctx, const double *x0, int64_t three_n, const double *r_max, double penalty, const double *prev, \
        const double *d_lim, double tan_half_fov, const mac_mads_params *prm, double *x_out, mac_mads_stats *st
#define MADS_RUN_PASS ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, x_out, st
#define MADS_BEGIN_ARGS                                                                                    \
    mac_ctx *ctx, const double *x0, int64_t three_n, const double *r_max, double penalty, const double *prev, \
        const double *d_lim, double tan_half_fov, const mac_mads_params *prm, int64_t shard_lo,            \
        int64_t shard_hi, mac_mads **out
#define MADS_BEGIN_PASS ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, shard_lo, shard_hi, out

int32_t mac_mads_run(MADS_RUN_ARGS) { return mads_run_impl(MADS_RUN_PASS, MadsSetup{}); }
int32_t mac_mads_run_cons(MADS_RUN_ARGS, const mac_cons* cons) { return mads_run_impl(MADS_RUN_PASS, MadsSetup{cons}); }
int32_t mac_mads_run_opts(MADS_RUN_ARGS, const mac_cons* cons, const mac_mads_opts* opts)
{
    return mads_run_impl(MADS_RUN_PASS, MadsSetup{cons, opts});
}
int32_t mac_mads_run_motion(MADS_RUN_ARGS, const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion)
{
    return mads_run_impl(MADS_RUN_PASS, MadsSetup{cons, opts, motion});
}
int32_t mac_mads_run_mesh(MADS_RUN_ARGS, const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion,
                          const mac_mads_mesh* mesh)
{
    return mads_run_impl(MADS_RUN_PASS, MadsSetup{cons, opts, motion, mesh});
}

int32_t mac_mads_begin(MADS_BEGIN_ARGS) { return mads_begin_impl(MADS_BEGIN_PASS, MadsSetup{}); }
int32_t mac_mads_begin_cons(MADS_BEGIN_ARGS, const mac_cons* cons)
{
    return mads_begin_impl(MADS_BEGIN_PASS, MadsSetup{cons});
}
int32_t mac_mads_begin_opts(MADS_BEGIN_ARGS, const mac_cons* cons, const mac_mads_opts* opts)
{
    return mads_begin_impl(MADS_BEGIN_PASS, MadsSetup{cons, opts});
}
int32_t mac_mads_begin_motion(MADS_BEGIN_ARGS, const mac_cons* cons, const mac_mads_opts* opts,
                              const mac_motion* motion)
{
    return mads_begin_impl(MADS_BEGIN_PASS, MadsSetup{cons, opts, motion});
}
int32_t mac_mads_begin_mesh(MADS_BEGIN_ARGS, const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion,
                            const mac_mads_mesh* mesh)
{
    return mads_begin_impl(MADS_BEGIN_PASS, MadsSetup{cons, opts, motion, mesh});
}
#undef MADS_RUN_ARGS
#undef MADS_RUN_PASS
#undef MADS_BEGIN_ARGS
#undef MADS_BEGIN_PASS

// The progressive barrier's loop (the rule: DESIGN.md section 4), stepped by the host from the
// stepper's pieces. Per iteration: one basis; per centre (F, then I) the staging copy, the mask
// launch (if any), prog_h_kernel and the poll chain on the stepper's stream, the first centre's
// objectives copied aside (K doubles, device to device) before the second chain overwrites them;
// then prog_select_kernel and one copy of its record with a stream synchronisation.
static void mads_run_prog_loop(mac_mads* m, const mac_prog* prog, double h0, double h_max, double* x_out,
                               double* x_inf_out, mac_mads_prog_stats* ps)
{
    mac_ctx* ctx = m->ctx;
    Lane* L = m->L;
    hipStream_t s = m->s;
    const int n = m->n, np = m->np, N = m->N, K = m->K;
    const ProgArgs pargs = prog_upload(L, s, N, prog);
    L->progh.reserve(sizeof(double) * 2 * (size_t)K);
    L->progobj.reserve(sizeof(double) * (size_t)K);
    L->progrec.reserve(sizeof(ProgRec));
    double* d_h[2] = {L->progh.as<double>(), L->progh.as<double>() + K};
    // pinned staging of this loop: per centre [centre 8n][permutations 4*2np][h fill 8K], the record
    const size_t stage_c = sizeof(double) * (size_t)n + sizeof(int) * 2 * (size_t)np;
    const size_t stage_sz = ((stage_c + 7) & ~(size_t)7) + sizeof(double) * (size_t)K;
    PinnedBuf stage;
    stage.reserve(2 * stage_sz + sizeof(ProgRec));
    struct Release {
        PinnedBuf& b;
        ~Release() { b.release(); }
    } release{stage};
    ProgRec* h_rec = reinterpret_cast<ProgRec*>((char*)stage.p + 2 * stage_sz);
    // a centre's xinc on the device: the lane's buffer holds both
    L->xinc.reserve(2 * ((stage_c + 255) & ~(size_t)255));
    char* d_xinc[2] = {(char*)L->xinc.p, (char*)L->xinc.p + ((stage_c + 255) & ~(size_t)255)};

    struct Inc {
        std::vector<double> x;
        double f = INFINITY, h = 0.0;
        bool has = false;
    } F, I;
    if (h0 == 0.0) {
        F.x = m->x;
        F.f = m->f;
        F.has = true;
    } else {
        I.x = m->x;
        I.f = m->f;
        I.h = h0;
        I.has = true;
    }
    int64_t n_dom = 0, n_imp = 0, n_uns = 0, two = 0, evaluated = 0;
    while (m->it < m->prm.n_iter && m->ell >= 0) {
        const auto ta = MadsClock::now();
        ++m->it;
        const int64_t b = (int64_t)1 << m->ell;
        m->rp.swap(m->rp_next);
        m->cp.swap(m->cp_next);
        const Inc* cen[2] = {nullptr, nullptr};
        int nc = 0;
        if (F.has) cen[nc++] = &F;
        if (I.has) cen[nc++] = &I;
        if (nc == 2) ++two;
        const double* sel_obj[2] = {nullptr, nullptr};   // (a centre cons3 rejected whole stays null)
        const double* sel_h[2] = {nullptr, nullptr};
        for (int c = 0; c < nc; ++c) {
            m->evals += K;
            if (poll_rejected(m, b, cen[c]->x.data())) {   // cons3 rejects the whole poll: no launch
                ++m->rejected;
                continue;
            }
            char* hs = (char*)stage.p + (size_t)c * stage_sz;
            const int* d_perm = mads_stage(m, cen[c]->x.data(), m->rp, m->cp, hs, d_xinc[c]);
            const CandSrc src = mads_gen_src(m, reinterpret_cast<const double*>(d_xinc[c]), d_perm, m->stream.state, b, 0);
            ProgLaunch pl{pargs, h_max, d_h[c]};
            if (m->xy) {   // the radii are held: every candidate's h is the centre's (<= h_max)
                double* hh = reinterpret_cast<double*>(hs + ((stage_c + 7) & ~(size_t)7));
                std::fill(hh, hh + K, cen[c]->h);
                HCK(hipMemcpyAsync(d_h[c], hh, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, s));
            }
            EvalReq rq = mads_request(m, src, K);
            rq.d_feas = m->d_feas.as<unsigned long long>();
            rq.prog = m->xy ? nullptr : &pl;
            enqueue_eval(ctx, L, s, rq);
            sel_h[c] = d_h[c];
            if (c == 0 && nc == 2) {
                HCK(hipMemcpyAsync(L->progobj.p, L->obj.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, s));
                sel_obj[c] = L->progobj.as<double>();
            } else {
                sel_obj[c] = L->obj.as<double>();
            }
        }
        prog_select_launch(s, prog_take_ts(ctx, kRoleProgSel, 1), sel_obj, sel_h, K, F.has, I.has, F.f, I.f, I.h,
                           h_max, L->progrec.as<ProgRec>());
        HCK(hipMemcpyAsync(h_rec, L->progrec.p, sizeof(ProgRec), hipMemcpyDeviceToHost, s));
        const auto tb = MadsClock::now();
        // the next iteration's permutations, while the device works
        if (m->it < m->prm.n_iter) m->stream.draw(m->stream.state_after(1), m->rp_next, m->cp_next);
        const auto tc = MadsClock::now();
        HCK(hipStreamSynchronize(s));
        const auto td = MadsClock::now();
        const ProgRec r = *h_rec;
        // candidate g = c K + k of this iteration: centre c moved along column k of the basis
        auto point = [&](int64_t g, std::vector<double>& out) {
            out.resize(n);
            mads_candidate(mads_poll_at(m, b, m->rp, m->cp), g % K, cen[g / K]->x.data(), n, out.data());
        };
        std::vector<double> xF, xI;
        const bool improves = (r.outcome & 256) != 0;
        if (improves) point(r.bestF_g, xF);
        if (r.newI_g >= 0) point(r.newI_g, xI);
        if (improves) {
            F.x.swap(xF);
            F.f = r.bestF_f;
            F.has = true;
        }
        if (r.newI_g >= 0) {
            I.x.swap(xI);
            I.f = r.newI_f;
            I.h = r.newI_h;
            I.has = true;
        } else if (r.newI_g == kProgNone) {
            I.has = false;
        }
        h_max = r.h_new;
        evaluated += r.evaluated;
        switch ((int)(r.outcome & 255)) {
        case 0:
            m->ell = std::min(m->ell + 1, (int)m->prm.ell_max);
            ++n_dom;
            ++m->succ;
            break;
        case 1:
            ++n_imp;
            break;
        default:
            --m->ell;
            ++n_uns;
        }
        m->stream.advance();
        const auto te = MadsClock::now();
        m->h_enq += mads_secs(ta, tb);
        m->h_perm += mads_secs(tb, tc);
        m->h_wait += mads_secs(tc, td);
        m->h_post += mads_secs(td, te);
    }
    const Inc& out = F.has ? F : I;
    m->x = out.x;
    m->f = out.f;
    std::copy(out.x.begin(), out.x.end(), x_out);
    if (x_inf_out && I.has) std::copy(I.x.begin(), I.x.end(), x_inf_out);
    if (ps) {
        ps->has_feasible = F.has ? 1 : 0;
        ps->has_infeasible = I.has ? 1 : 0;
        ps->f_feasible = F.has ? F.f : INFINITY;
        ps->f_infeasible = I.has ? I.f : INFINITY;
        ps->h_infeasible = I.has ? I.h : 0.0;
        ps->h_max = h_max;
        ps->dominating = n_dom;
        ps->improving = n_imp;
        ps->unsuccessful = n_uns;
        ps->two_centre_polls = two;
        ps->evaluated = evaluated;
    }
}

int32_t mac_mads_run_prog(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                          double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                          const mac_mads_params* prm, double* x_out, mac_mads_stats* st, const mac_cons* cons,
                          const mac_mads_opts* opts, const mac_motion* motion, const mac_mads_mesh* mesh,
                          const mac_prog* prog, double* x_inf_out, mac_mads_prog_stats* pstats)
{
    ABI_BEGIN
    bool on = false;
    int32_t rc = prog_check(prog, three_n, &on);
    if (rc) return rc;
    MadsSetup su{cons, opts, motion, mesh};
    if (!on)   // no progressive constraint: the _mesh call
        return mads_run_impl(ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, x_out, st, su);
    if (!x0 || !x_out) return fail(MAC_E_INVAL, "null argument");
    const int N = (int)(three_n / 3);
    const double h0 = prog_h_host(x0, N, prog);
    if (h0 != h0) return fail(MAC_E_INVAL, "mac_prog: h(x0) is NaN");
    const bool given = prog->h_max0 >= 0.0;   // (NaN: false)
    const double h_max = given ? prog->h_max0 : (h0 > 0.0 ? h0 : (double)INFINITY);
    if (h0 > h_max)
        return fail(MAC_E_INVAL, "mac_prog: h(x0) = " + std::to_string(h0) + " > h_max0 = " + std::to_string(h_max));
    rc = mads_setup_check(su, three_n);
    if (rc) return rc;
    su.prog = true;   // (MAC_OPT_VERDICTS is ignored)
    mac_mads* m = nullptr;
    rc = mads_begin_impl(ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, 0,
                         mads_poll_count(three_n, su.xy), &m, su);
    if (rc) return rc;
    try {
        set_device(ctx);
        mads_run_prog_loop(m, prog, h0, h_max, x_out, x_inf_out, pstats);
    } catch (...) {
        mac_mads_destroy(m);
        throw;
    }
    rc = mac_mads_result(m, nullptr, st);
    mac_mads_destroy(m);
    return rc;
    ABI_END
}

// ------------------------------------------------------------------ the progressive barrier as a stepper
// mac_mads_run_prog's loop one iteration at a time over the shard [lo, hi) of every centre's poll
// (mac_mads_begin_prog / _poll_prog / _advance_prog / _result_prog): a poll reports the shard-partial
// record of prog_rule.h (prog_part_kernel, one pass), the ranks merge their records (mac_prog_merge: exact,
// in any order) and all apply the merged one, so they hold the single-GPU loop's F, I and h_max. A poll
// `ahead` iterations on assumes that the iterations between are unsuccessful and leave I as it is
// (prog_chains): the same centres, ell - ahead, the threshold such an iteration leaves.
static_assert(sizeof(mac_prog_part) == sizeof(ProgPart), "mac_prog_part is ProgPart");

int32_t mac_mads_begin_prog(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max, double penalty,
                            const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* prm, int64_t shard_lo, int64_t shard_hi, mac_mads** out,
                            const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion,
                            const mac_mads_mesh* mesh, const mac_prog* prog)
{
    ABI_BEGIN
    if (out) *out = nullptr;
    bool on = false;
    int32_t rc = prog_check(prog, three_n, &on);
    if (rc) return rc;
    MadsSetup su{cons, opts, motion, mesh};
    if (!on)   // no progressive constraint: the _mesh call
        return mads_begin_impl(ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, shard_lo, shard_hi,
                               out, su);
    if (!x0 || !out) return fail(MAC_E_INVAL, "null argument");
    const int N = (int)(three_n / 3);
    const double h0 = prog_h_host(x0, N, prog);
    if (h0 != h0) return fail(MAC_E_INVAL, "mac_prog: h(x0) is NaN");
    const bool given = prog->h_max0 >= 0.0;   // (NaN: false)
    const double h_max = given ? prog->h_max0 : (h0 > 0.0 ? h0 : (double)INFINITY);
    if (h0 > h_max)
        return fail(MAC_E_INVAL, "mac_prog: h(x0) = " + std::to_string(h0) + " > h_max0 = " + std::to_string(h_max));
    rc = mads_setup_check(su, three_n);
    if (rc) return rc;
    su.prog = true;   // (MAC_OPT_VERDICTS is ignored)
    mac_mads* m = nullptr;
    rc = mads_begin_impl(ctx, x0, three_n, r_max, penalty, prev, d_lim, tan_half_fov, prm, shard_lo, shard_hi, &m, su);
    if (rc) return rc;
    try {
        set_device(ctx);
        Lane* L = m->L;
        const size_t Kc = (size_t)(m->hi - m->lo);
        MadsProg* pg = m->pg = new MadsProg();
        pg->pargs = prog_upload(L, m->s, N, prog);
        HCK(hipStreamSynchronize(m->s));   // (the caller's arrays may go once the call returns)
        L->progh.reserve(sizeof(double) * 2 * std::max<size_t>(Kc, 1));
        L->progobj.reserve(sizeof(double) * std::max<size_t>(Kc, 1));
        L->progrec.reserve(sizeof(ProgPart));
        pg->d_h[0] = L->progh.as<double>();
        pg->d_h[1] = L->progh.as<double>() + Kc;
        pg->stage_c = sizeof(double) * (size_t)m->n + sizeof(int) * 2 * (size_t)m->np;
        pg->stage_sz = ((pg->stage_c + 7) & ~(size_t)7) + sizeof(double) * Kc;
        pg->stage.reserve(2 * pg->stage_sz + sizeof(ProgPart));
        pg->h_part = reinterpret_cast<ProgPart*>((char*)pg->stage.p + 2 * pg->stage_sz);
        const size_t xinc_c = (pg->stage_c + 255) & ~(size_t)255;   // a centre's xinc: the lane's buffer holds both
        L->xinc.reserve(2 * xinc_c);
        pg->d_xinc[0] = (char*)L->xinc.p;
        pg->d_xinc[1] = (char*)L->xinc.p + xinc_c;
        ProgInc& inc = h0 == 0.0 ? pg->F : pg->I;
        inc.x = m->x;
        inc.f = m->f;
        inc.h = h0;
        inc.has = true;
        pg->h_max = h_max;
    } catch (...) {
        mac_mads_destroy(m);
        throw;
    }
    *out = m;
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_poll_prog(mac_mads* m, int32_t ahead, int32_t* done, mac_prog_part* part)
{
    ABI_BEGIN
    if (!m || !done || !part) return fail(MAC_E_INVAL, "null argument");
    if (!m->pg) return fail(MAC_E_INVAL, "mac_mads_poll_prog on a stepper without a prog (use mac_mads_poll)");
    if (ahead < 0) return fail(MAC_E_INVAL, "negative ahead");
    MadsProg* pg = m->pg;
    *done = 0;
    const int64_t tag = m->it + ahead + 1;
    ProgPart pp = prog_part_empty(tag);
    if (m->it + ahead >= m->prm.n_iter || m->ell - ahead < 0) {
        *done = 1;
        pp.tag |= kProgTagDone;
        std::memcpy(part, &pp, sizeof(pp));
        return MAC_OK;
    }
    const int Kc = (int)(m->hi - m->lo);
    if (Kc == 0) {   // an empty shard: no launch, the empty record
        std::memcpy(part, &pp, sizeof(pp));
        return MAC_OK;
    }
    set_device(m->ctx);
    mac_ctx* ctx = m->ctx;
    Lane* L = m->L;
    hipStream_t s = m->s;
    const auto ta = MadsClock::now();
    const int64_t b = (int64_t)1 << (m->ell - ahead);
    const uint64_t state = m->stream.state_after((uint64_t)ahead);
    std::vector<int> rp_a, cp_a;   // (ahead = 0: the current iteration's permutations are computed already)
    if (ahead > 0) m->stream.draw(state, rp_a, cp_a);
    const std::vector<int>& rp = ahead > 0 ? rp_a : m->rp_next;
    const std::vector<int>& cp = ahead > 0 ? cp_a : m->cp_next;
    // what an unsuccessful iteration leaves: h_max = I.h with an I, else as it was
    ProgScalars sc = pg->scalars();
    if (ahead > 0 && pg->I.has) sc.h_max = pg->I.h;
    const ProgInc* cen[2] = {nullptr, nullptr};
    int nc = 0;
    if (pg->F.has) cen[nc++] = &pg->F;
    if (pg->I.has) cen[nc++] = &pg->I;
    const double* sel_obj[2] = {nullptr, nullptr};   // (a centre cons3 rejected whole stays null)
    const double* sel_h[2] = {nullptr, nullptr};
    bool any = false;
    for (int c = 0; c < nc; ++c) {
        if (poll_rejected(m, b, cen[c]->x.data())) continue;   // (counted by mac_mads_advance_prog once applied)
        char* hs = (char*)pg->stage.p + (size_t)c * pg->stage_sz;
        const int* d_perm = mads_stage(m, cen[c]->x.data(), rp, cp, hs, pg->d_xinc[c]);
        const CandSrc src = mads_gen_src(m, reinterpret_cast<const double*>(pg->d_xinc[c]), d_perm, state, b, (int)m->lo);
        ProgLaunch pl{pg->pargs, sc.h_max, pg->d_h[c]};
        if (m->xy) {   // the radii are held: every candidate's h is the centre's (<= h_max)
            double* hh = reinterpret_cast<double*>(hs + ((pg->stage_c + 7) & ~(size_t)7));
            std::fill(hh, hh + Kc, cen[c]->h);
            HCK(hipMemcpyAsync(pg->d_h[c], hh, sizeof(double) * (size_t)Kc, hipMemcpyHostToDevice, s));
        }
        EvalReq rq = mads_request(m, src, Kc);
        rq.d_feas = m->d_feas.as<unsigned long long>();
        rq.prog = m->xy ? nullptr : &pl;
        enqueue_eval(ctx, L, s, rq);
        sel_h[c] = pg->d_h[c];
        if (c == 0 && nc == 2) {
            HCK(hipMemcpyAsync(L->progobj.p, L->obj.p, sizeof(double) * (size_t)Kc, hipMemcpyDeviceToDevice, s));
            sel_obj[c] = L->progobj.as<double>();
        } else {
            sel_obj[c] = L->obj.as<double>();
        }
        any = true;
    }
    const auto tb = MadsClock::now();
    if (any) {
        prog_part_launch(s, prog_take_ts(ctx, kRoleProgSel, 1), sel_obj, sel_h, Kc, m->K, m->lo, tag, sc,
                         L->progrec.as<ProgPart>());
        HCK(hipMemcpyAsync(pg->h_part, L->progrec.p, sizeof(ProgPart), hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        pp = *pg->h_part;
    }
    std::memcpy(part, &pp, sizeof(pp));
    m->h_enq += mads_secs(ta, tb);
    m->h_wait += mads_secs(tb, MadsClock::now());
    return MAC_OK;
    ABI_END
}

int32_t mac_prog_merge(const mac_prog_part* parts, int32_t n, mac_prog_part* out)
{
    ABI_BEGIN
    if (!parts || !out) return fail(MAC_E_INVAL, "null argument");
    if (n < 1) return fail(MAC_E_INVAL, "mac_prog_merge: no record");
    ProgPart acc;
    std::memcpy(&acc, &parts[0], sizeof(acc));
    for (int32_t q = 1; q < n; ++q) {
        ProgPart p;
        std::memcpy(&p, &parts[q], sizeof(p));
        if (p.tag != acc.tag)
            return fail(MAC_E_INVAL, "mac_prog_merge: records of different iterations (tags " +
                                         std::to_string(acc.tag) + " and " + std::to_string(p.tag) + ")");
        prog_part_merge(acc, p);
    }
    std::memcpy(out, &acc, sizeof(acc));
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_advance_prog(mac_mads* m, const mac_prog_part* merged, int32_t* outcome, int32_t* chains)
{
    ABI_BEGIN
    if (!m || !merged) return fail(MAC_E_INVAL, "null argument");
    if (!m->pg) return fail(MAC_E_INVAL, "mac_mads_advance_prog on a stepper without a prog (use mac_mads_advance)");
    if (m->it >= m->prm.n_iter || m->ell < 0) return fail(MAC_E_INVAL, "mac_mads_advance_prog past the loop's end");
    MadsProg* pg = m->pg;
    ProgPart pp;
    std::memcpy(&pp, merged, sizeof(pp));
    if (pp.tag != m->it + 1)
        return fail(MAC_E_INVAL, "mac_mads_advance_prog: the record's tag " + std::to_string(pp.tag) +
                                     " is not iteration " + std::to_string(m->it + 1));
    const auto t0 = MadsClock::now();
    const int n = m->n, K = m->K;
    const int64_t b = (int64_t)1 << m->ell;
    const ProgInc* cen[2] = {nullptr, nullptr};
    int nc = 0;
    if (pg->F.has) cen[nc++] = &pg->F;
    if (pg->I.has) cen[nc++] = &pg->I;
    const bool had_I = pg->I.has;
    const ProgRec r = prog_finish(pp, pg->scalars());
    const bool improves = (r.outcome & 256) != 0;
    const int64_t top = (int64_t)nc * K;
    if ((improves && r.bestF_g >= top) || r.newI_g >= top)
        return fail(MAC_E_INVAL, "mac_mads_advance_prog: a candidate index outside the polls");
    ++m->it;
    if (nc == 2) ++pg->two;
    for (int c = 0; c < nc; ++c) {
        m->evals += K;
        // the applied poll's whole-poll rejection, decided as mac_mads_poll_prog does
        if (m->hi > m->lo && poll_rejected(m, b, cen[c]->x.data())) ++m->rejected;
    }
    // candidate g = c K + k of this iteration: centre c moved along column k of the basis
    // (the current iteration's permutations: rp_next / cp_next)
    auto point = [&](int64_t g, std::vector<double>& out) {
        out.resize(n);
        mads_candidate(mads_poll_at(m, b, m->rp_next, m->cp_next), g % K, cen[g / K]->x.data(), n, out.data());
    };
    std::vector<double> xF, xI;
    if (improves) point(r.bestF_g, xF);
    if (r.newI_g >= 0) point(r.newI_g, xI);
    if (improves) {
        pg->F.x.swap(xF);
        pg->F.f = r.bestF_f;
        pg->F.has = true;
    }
    if (r.newI_g >= 0) {
        pg->I.x.swap(xI);
        pg->I.f = r.newI_f;
        pg->I.h = r.newI_h;
        pg->I.has = true;
    } else if (r.newI_g == kProgNone) {
        pg->I.has = false;
    }
    pg->h_max = r.h_new;
    pg->evaluated += r.evaluated;
    switch ((int)(r.outcome & 255)) {
    case 0:
        m->ell = std::min(m->ell + 1, (int)m->prm.ell_max);
        ++pg->n_dom;
        ++m->succ;
        break;
    case 1:
        ++pg->n_imp;
        break;
    default:
        --m->ell;
        ++pg->n_uns;
    }
    m->stream.advance();
    if (m->it < m->prm.n_iter) m->stream.draw(m->stream.state, m->rp_next, m->cp_next);
    if (outcome) *outcome = (int32_t)(r.outcome & 255);
    if (chains) *chains = prog_chains(r, had_I) ? 1 : 0;
    m->h_post += mads_secs(t0, MadsClock::now());
    return MAC_OK;
    ABI_END
}

int32_t mac_mads_result_prog(mac_mads* m, double* x_out, double* x_inf_out, mac_mads_stats* st,
                             mac_mads_prog_stats* ps)
{
    ABI_BEGIN
    if (!m) return fail(MAC_E_INVAL, "null stepper");
    if (!m->pg) return fail(MAC_E_INVAL, "mac_mads_result_prog on a stepper without a prog (use mac_mads_result)");
    const MadsProg* pg = m->pg;
    const ProgInc& out = pg->F.has ? pg->F : pg->I;
    m->x = out.x;
    m->f = out.f;
    if (x_inf_out && pg->I.has) std::copy(pg->I.x.begin(), pg->I.x.end(), x_inf_out);
    if (ps) {
        ps->has_feasible = pg->F.has ? 1 : 0;
        ps->has_infeasible = pg->I.has ? 1 : 0;
        ps->f_feasible = pg->F.has ? pg->F.f : INFINITY;
        ps->f_infeasible = pg->I.has ? pg->I.f : INFINITY;
        ps->h_infeasible = pg->I.has ? pg->I.h : 0.0;
        ps->h_max = pg->h_max;
        ps->dominating = pg->n_dom;
        ps->improving = pg->n_imp;
        ps->unsuccessful = pg->n_uns;
        ps->two_centre_polls = pg->two;
        ps->evaluated = pg->evaluated;
    }
    return mac_mads_result(m, x_out, st);
    ABI_END
}

}  // extern "C"
