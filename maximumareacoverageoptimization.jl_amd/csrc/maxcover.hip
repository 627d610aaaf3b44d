// maxcover.hip — libmaxcover: context, device-resident point list, and the C-ABI declared in
// include/maxcover.h. gfx950 only (hipcc --offload-arch=gfx950).
//
// Reference seam: src/TDM_STATIC_opt.jl:82-100 (AreaMaxObjective / createObjective) and
// src/AreaCoverageCalculation.jl:63-110 (calculateArea). See DESIGN.md.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <sched.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <hipcub/hipcub.hpp>
#include <immintrin.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <thread>
#include <vector>

#include "kernels.h"
#include "maxcover.h"

#pragma clang fp contract(off)

using namespace mac;

static constexpr int kPollMinK = 64;          // below this the per-candidate walk always wins
static constexpr int kTiledMaxN = 2048;       // the per-candidate walk keeps all N disks in LDS;
                                              // more UAVs take the poll walk at any K (one
                                              // workgroup per disk: a per-disk walk for K = 1)
static constexpr double kPollCostRatio = 4.0; // poll walk if its visits <= 4x the other's

// (host only, this file's own: they read the constants above and the kernels' names unqualified)
#include "eval_plan.h"
#include "kernel_select.h"

// ------------------------------------------------------------------ errors

static thread_local std::string g_last_error;

static int32_t fail(int32_t code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

struct HipError {
    hipError_t e;
    const char* what;
    int line;
    const char* file = "maxcover.hip";   // (mads_driver.h's checks name their own file)
};

#define HCK(expr)                                              \
    do {                                                       \
        hipError_t _e = (expr);                                \
        if (_e != hipSuccess) throw HipError{_e, #expr, __LINE__, __FILE_NAME__}; \
    } while (0)

#define ABI_BEGIN try {
#define ABI_END                                                                               \
    }                                                                                         \
    catch (const HipError& he) {                                                              \
        char buf[512];                                                                        \
        snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d in %s", (int)he.e,               \
                 hipGetErrorString(he.e), he.file, he.line, he.what);                         \
        return fail(he.e == hipErrorOutOfMemory ? MAC_E_NOMEM : MAC_E_HIP, buf);              \
    }                                                                                         \
    catch (const std::bad_alloc&) {                                                           \
        return fail(MAC_E_NOMEM, "host allocation failed");                                   \
    }                                                                                         \
    catch (...) {                                                                             \
        return fail(MAC_E_HIP, "unexpected exception");                                       \
    }

// ------------------------------------------------------------------ device buffers

// hipFree / hipHostFree synchronise the device. While an armed poll's stream wait is enqueued
// ahead of its own launches (mac_poll_arm_dev_f64), a buffer that grows must not be freed there:
// the wait only opens after the arming call returns, so the device would never drain. Frees on
// the arming thread go to this list instead ({pointer, pinned}) and are released at the next
// call that synchronises the device anyway (point-list changes, mac_ctx_destroy).
static thread_local std::vector<std::pair<void*, bool>>* t_defer_free = nullptr;

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    // fine: fine-grained device memory (host-writable through a large BAR: the closure's
    // candidates, closure_launch)
    void reserve(size_t bytes, bool fine = false)
    {
        if (bytes <= cap) return;
        if (p && t_defer_free)
            t_defer_free->push_back({p, false});
        else if (p)
            HCK(hipFree(p));
        p = nullptr;
        cap = 0;
        size_t b = bytes < 256 ? 256 : bytes;
        b = (b + 255) & ~(size_t)255;
        if (fine)
            HCK(hipExtMallocWithFlags(&p, b, hipDeviceMallocFinegrained));
        else
            HCK(hipMalloc(&p, b));
        cap = b;
    }
    // reserve(); true when the buffer was (re)allocated (its contents are then undefined)
    bool grow(size_t bytes)
    {
        if (bytes <= cap) return false;
        reserve(bytes);
        return true;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

// Page-locked host staging owned by a lane (async copies must not target pageable memory, or
// HIP performs them synchronously).
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    void reserve(size_t b, unsigned flags = hipHostMallocDefault)
    {
        if (b <= cap) return;
        if (p && t_defer_free)
            t_defer_free->push_back({p, true});
        else if (p)
            HCK(hipHostFree(p));
        p = nullptr;
        cap = 0;
        HCK(hipHostMalloc(&p, b, flags));
        cap = b;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Per-call scratch + stream ("lane"); lanes are pooled so concurrent host threads each get one.
struct Lane {
    hipStream_t stream = nullptr;
    hipStream_t last = nullptr;   // stream of the most recent use
    hipEvent_t done = nullptr;
    DevBuf cands, disks, partial, area, obj, best, rmax, prev, dlim, region, mode, nbr,
        ncount, dlist, spart, vp, xinc, perm, ucount, umap, keysT, lane4, lanexp, rows, nboxT,
        cnt, dlimraw, finblk, finarrive, c32, p32, qual, nboxU, ncountU, orjobs;
    std::vector<double> h_dlim;
    PinnedBuf h_stage;                         // native MADS driver: best, permutations, incumbent
    PinnedBuf h_io;                            // host-pointer calls: candidates in, results out
    PinnedBuf h_dc;                            // disks with neighbours of the last poll (mapped)
    int* d_dc = nullptr;                       // ... its device address
    int dc_hist[8] = {};                       // ... as read at the last 8 poll enqueues
    PinnedBuf h_cl;                            // closure_kernel's result slot (mapped)
    uint64_t* d_cl = nullptr;                  // ... its device address
    uint64_t cl_seq = 0;
    DevBuf cpart, carrive, ctot;               // closure_kernel: credits, arrivals, packed count
    DevBuf clv;                                // closure candidates written by the host (BAR)
    DevBuf bdpart, bdarrive, bdout;            // by_disk_kernel: owned words, arrivals; host calls' results
    DevBuf cmask, cbest;                       // masked poll (k_cons.h): feasibility bytes; the chain's own best
    DevBuf motion;                             // mac_motion's per-UAV arrays (k_cons.h MotionArgs): 8N doubles
    DevBuf verdict;                            // verdict records (k_cons.h Verdict): 64 B per candidate
    DevBuf prog, progh, progobj, progrec;      // mac_prog (k_prog.h): member and limit; h and the first centre's
                                               // objectives of an iteration; prog_select_kernel's record
    std::vector<double> h_motion;              // ... as built on the host
    DevBuf prec, cost;                         // prep launch: per-disk records; walk costs
    int um_hist[8] = {};                       // most distinct positions of a disk, last 8 polls
    int walk_hist[8] = {};                     // the walk AUTO would have chosen, last 8 polls
    // the fused chain (k_fiw.h): displacement partials, failure bytes, credit rows, hint words,
    // the shared entries handed to fin2_kernel
    DevBuf pd, dead8, frows, fwhint, fwlist, fwcount, fwsxy, fwsw;
    int last_chain = 0;                        // the chain of the lane's last poll: 1 five-launch, 2 fused
};

// RCCL's C API, bound at run time from the librccl the process already uses (torch's, or the
// system one): the multi-GPU poll exchange (mac_poll_exchange) issues its all-gather on the poll's
// own stream. The few types it needs, by their published layout (rccl.h): ncclUniqueId is 128
// opaque bytes, ncclComm_t a pointer, ncclUint8 = 1, ncclSuccess = 0.
struct RcclUid {
    char internal[128];
};
struct RcclApi {
    void* lib = nullptr;
    int (*get_unique_id)(RcclUid*) = nullptr;
    int (*comm_init_rank)(void**, int, RcclUid, int) = nullptr;
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*comm_destroy)(void*) = nullptr;
    const char* (*error_string)(int) = nullptr;
};

struct mac_ctx {
    int device = 0;
    int cus = 256;
    std::mutex mu;
    // MAXCOVER_HOST_STATS=1: host time of a device poll call, split at its launches (printed at
    // destroy): [0] entry -> prep launch call, [1] prep launch, [2] fiw launch, [3] fin2 launch
    bool host_stats = false;
    double hs_t[4] = {0, 0, 0, 0};
    int64_t hs_n = 0;
    // the multi-GPU poll exchange (mac_comm_init): an RCCL communicator over the node's ranks and
    // the world x 16-B gather buffer
    RcclApi* rccl = nullptr;
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    void* d_xrec = nullptr;
    std::mutex xmu;          // mac_exchange_records: its staging
    PinnedBuf h_xrec;        // [own record 256 B][world records]
    void* d_xrec2 = nullptr;
    // the fused chain's routing history over every lane's polls (enqueue_eval): bit q set when the
    // q-th last reported poll did not suit it (a workload property: a MADS stepper or a new lane
    // takes it over from the lanes before it)
    std::atomic<uint64_t> fused_bad{0};
    std::atomic<bool> route_seeded{false};   // the first matrix poll's routing from the poll (seed_route)
    // mac_area_f64's combiner: queued single-candidate requests, one batch launch at a time
    std::mutex cl_mu;
    std::deque<struct ClReq*> cl_q;
    std::atomic<int> cl_busy{0};   // batches being launched (changed under cl_mu; read as a hint)
    std::atomic<int> cl_active{0};   // callers inside mac_area_f64's combiner
    int cl_taken = 0;                // requests in batches in flight (under cl_mu)
    // queued callers sleep on the futex word of their generation (the batches taken since the
    // context began, cl_gen: every request queued between two takes is in the second's batch)
    std::atomic<uint32_t> cl_gen{0};     // (changed under cl_mu)
    std::atomic<int> cl_genw[64] = {};
    int64_t cl_batches = 0, cl_reqs = 0;   // (MAXCOVER_CL_STATS=1: printed at destroy)
    // MAXCOVER_CL_STATS=1 (nanoseconds, relaxed adds: no lock on the combiner's path)
    std::atomic<int64_t> cl_phase_ns[4] = {};   // per batch: staging, copy + launch enqueued, hand-out, lane
    std::atomic<int64_t> cl_req_ns[5] = {};     // per request: queued -> taken -> handed out -> seen ->
                                                // slot read; the call
    std::atomic<int64_t> cl_led{0};             // requests whose own thread led their batch
    std::vector<Lane*> lanes_free;
    std::vector<Lane*> lanes_all;
    std::atomic<Lane*> last_five{nullptr};   // the lane of the most recent five-launch poll (mac_diag_poll_report)
    hipStream_t setup_stream = nullptr;
    // device polls' result mirror (guarded by mu): one mapped coherent slot {obj bits, index,
    // seq, check} per d_best buffer (k_final.h mirror_check), reassigned least recently used; the
    // finalize of a device poll writes its result into its d_best's slot under a fresh seq
    static constexpr int kMirrorSlots = 64;
    PinnedBuf h_mirror;
    uint64_t* d_mirror = nullptr;
    const void* mirror_key[kMirrorSlots] = {};
    uint64_t mirror_want[kMirrorSlots] = {};
    uint64_t mirror_used[kMirrorSlots] = {};
    uint64_t mirror_seq = 0, mirror_clock = 0;
    // armed polls (mac_poll_arm_dev_f64): the doorbell the streams wait on (coherent host memory), the
    // last ticket armed and the last released (the doorbell's value), tickets voided by a failed
    // arm that are released once every earlier ticket is, and each stream's latest armed ticket
    // (guarded by mu)
    uint64_t* doorbell = nullptr;
    uint64_t armed = 0, fired = 0;
    std::vector<uint64_t> voided;
    std::vector<std::pair<hipStream_t, uint64_t>> armed_on;
    // buffers an arming call replaced (t_defer_free), freed at the next device synchronisation
    std::vector<std::pair<void*, bool>> deferred;

    int algo = MAC_ALGO_AUTO;
    int shared_mode = MAC_SHARED_AUTO;   // MAC_OPT_SHARED
    int chain = MAC_CHAIN_AUTO;          // MAC_OPT_CHAIN
    int mesh_keys = MAC_KEYS_VALUE;      // MAC_OPT_MESH_KEYS (read when a MADS run or stepper begins)
    // MAC_OPT_VERDICTS (read when a MADS run or stepper begins): the tally the generated polls' explain
    // launches add to (k_cons.h kVerdictTally words; allocated by the first stepper that needs it, under
    // mu) and the launches tallied (counted on the host: mac_verdict_read)
    std::atomic<int> verdicts{0};
    DevBuf vtally;
    std::atomic<int64_t> verdict_polls{0};
    bool profile = false;
    // In-kernel launch timing (k_common.h ts_begin / ts_end): each profiled walk launch takes
    // nwg consecutive {start, end} slots of `stamps`. a: the scan / tiled launch, b: the poll
    // launch when the device picks the walk (mode != null): the launch that ran is read.
    // c / f: the chain's first launch (the prep) and its last (finalize), whose
    // stamps give the whole poll chain's device span (-1: not stamped)
    // (role stamps, mac_profile_kernels: [r] = {first slot, slots} of launch role r, -1: none; a poll
    // chain's launches take their stamps under their roles, and a, b, c, f are read off them when
    // the call is recorded: EvalRun::prof_end)
    struct Prof { int64_t a, na, b, nb; int64_t K; const int* mode; int algo;
                  int64_t c = -1, nc = 0, f = -1, nf = 0;
                  int64_t role[MAC_PROF_ROLES][2] = {{-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0},
                                                     {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0},
                                                     {-1, 0}, {-1, 0}}; };
    std::vector<Prof> prof;                          // recorded launches (guarded by mu)
    DevBuf stamps;
    int64_t stamp_cap = 0, stamp_used = 0;           // in workgroup slots (guarded by mu)
    int storage = MAC_STORE_F64;
    int tile_ppt = 4;

    int64_t M = 0;
    bool has_points = false;
    // original (list) order
    DevBuf x, y, w;
    // tile-sorted order
    DevBuf xys, ws, perm, off;
    Grid grid{};
    int64_t nTiles = 1;
    bool w_uniform = false;   // every entry's weight is bit-identical to w0 (build_index)
    // the host writes closure candidates straight into fine-grained device memory (a large-BAR
    // device: no host-to-device copy per closure batch); MAXCOVER_CL_BAR=0 turns it off
    std::atomic<bool> cl_bar{false};
    double w0 = 0.0;
    // setup scratch
    DevBuf keys_in, keys_out, idx_in, tmp, bbox, flags_s, flags_o, keep, sel_count, cx, cy, cw,
        cidx, circ, cdisk;
    // high-interest regions (mac_set_regions, k_regions.h): the boxes ([x_LB | x_UB | y_LB | y_UB],
    // kRegionsMax each; unused slots NaN) on the host and the device, the weight arriving entries
    // inside them get (NaN: left alone), the ingest counters (per box, then the union) and the
    // stats call's items, partials and results. n_regions = 0: off, nothing is launched
    int n_regions = 0;
    double reg_w_high = NAN;
    double h_boxes[4 * kRegionsMax];
    DevBuf rboxes, rcount, ritems, rpart, rout;
    // (profiling on) the fused chain's reports as the next enqueue read them (mac_profile_fused):
    // reports read, and the sum and the largest of hint word 1, the disks that took one position per
    // candidate (k_fiw.h kFwHints)
    std::atomic<int64_t> fw_reports{0}, fw_ident_sum{0}, fw_ident_max{0};
};

static void set_device(mac_ctx* ctx) { HCK(hipSetDevice(ctx->device)); }

// Free the buffers arming calls replaced; only after the device has been synchronised (every
// armed poll fired and drained).
static void free_deferred(mac_ctx* ctx)
{
    std::vector<std::pair<void*, bool>> v;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        v.swap(ctx->deferred);
    }
    for (auto& d : v) (void)(d.second ? hipHostFree(d.first) : hipFree(d.first));
}

// A lane's scratch may be reused at once by a call ordered on the SAME stream (stream order
// protects it; `ordered`: the *_dev calls, where `want` may be the null stream 0); on another
// stream only after the lane's last work has completed.
static Lane* acquire_lane(mac_ctx* ctx, hipStream_t want, bool ordered = false)
{
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ordered) {
            for (size_t i = 0; i < ctx->lanes_free.size(); ++i) {
                Lane* l = ctx->lanes_free[i];
                if (l->last == want) {
                    ctx->lanes_free.erase(ctx->lanes_free.begin() + (long)i);
                    return l;
                }
            }
        }
        for (size_t i = 0; i < ctx->lanes_free.size(); ++i) {
            Lane* l = ctx->lanes_free[i];
            if (hipEventQuery(l->done) == hipSuccess) {
                ctx->lanes_free.erase(ctx->lanes_free.begin() + (long)i);
                return l;
            }
        }
    }
    Lane* l = new Lane();
    HCK(hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking));
    HCK(hipEventCreateWithFlags(&l->done, hipEventDisableTiming));
    HCK(hipEventRecord(l->done, l->stream));
    l->last = l->stream;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->lanes_all.push_back(l);
    return l;
}

static void release_lane(mac_ctx* ctx, Lane* l, hipStream_t used)
{
    (void)hipEventRecord(l->done, used);
    l->last = used;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->lanes_free.push_back(l);
}

// Host-pointer calls: a lane on its own stream (synchronised before return).
// Device-pointer calls: the caller's stream; NULL is HIP's null stream, as in every HIP API, so a
// poll is ordered after the caller's default-stream work (torch's default stream is that stream).
// While an armed poll is not fired, no call may free a buffer it outgrows (t_defer_free): the
// free would wait for the device, which waits for the doorbell.
struct DeferFrees {
    mac_ctx* ctx;
    std::vector<std::pair<void*, bool>> v;
    bool on = false;
    explicit DeferFrees(mac_ctx* c) : ctx(c)
    {
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            on = ctx->armed > ctx->fired && !t_defer_free;
        }
        if (on) t_defer_free = &v;
    }
    ~DeferFrees()
    {
        if (!on) return;
        t_defer_free = nullptr;
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->deferred.insert(ctx->deferred.end(), v.begin(), v.end());
    }
};

struct LaneGuard {
    mac_ctx* ctx;
    DeferFrees df;
    Lane* lane;
    hipStream_t used;
    explicit LaneGuard(mac_ctx* c) : ctx(c), df(c), lane(acquire_lane(c, nullptr)), used(lane->stream) {}
    LaneGuard(mac_ctx* c, hipStream_t s) : ctx(c), df(c), lane(acquire_lane(c, s, true)), used(s) {}
    ~LaneGuard() { release_lane(ctx, lane, used); }
};

// A mapped result slot {obj bits, index, seq, check} (k_final.h) read once: true when it holds
// seq `want` and its check word matches (else its stores are still landing, or it is another
// poll's).
static bool mirror_read(const uint64_t* h, uint64_t want, double* obj, int64_t* idx, uint64_t* feas = nullptr)
{
    if (__atomic_load_n(h + 2, __ATOMIC_ACQUIRE) != want) return false;
    const uint64_t o = __atomic_load_n(h + 0, __ATOMIC_ACQUIRE);
    const uint64_t i = __atomic_load_n(h + 1, __ATOMIC_ACQUIRE);
    const uint64_t c = __atomic_load_n(h + 3, __ATOMIC_ACQUIRE);
    const uint64_t f = feas ? __atomic_load_n(h + 4, __ATOMIC_ACQUIRE) : 0;
    if (c != mirror_check(o, i, want, f) || __atomic_load_n(h + 2, __ATOMIC_ACQUIRE) != want) return false;
    *obj = __builtin_bit_cast(double, o);
    *idx = (int64_t)i;
    if (feas) *feas = f;
    return true;
}

// Spin on a slot for up to `ms` milliseconds.
static bool mirror_wait(const uint64_t* h, uint64_t want, double ms, double* obj, int64_t* idx,
                        uint64_t* feas = nullptr)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        if (mirror_read(h, want, obj, idx, feas)) return true;
        if ((spin & 1023) == 1023 &&
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > ms)
            return false;
    }
}

static inline unsigned grid1d(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// The lane's launch hints, mapped host words the poll kernels write for the next poll's enqueue:
// [0] disks with neighbours, [2] most positions of a disk, [4] the walk AUTO would choose (the
// five-launch chain, k_poll.h); [8..11] the fused chain's report (k_fiw.h kFwHints; -1: none yet)
static void ensure_hints(Lane* L)
{
    if (L->h_dc.p) return;
    L->h_dc.reserve(64, hipHostMallocMapped | hipHostMallocCoherent);
    volatile int* h = (volatile int*)L->h_dc.p;
    for (int q = 0; q < 16; ++q) h[q] = 0;
    h[0] = 1 << 30;   // first poll: launch
    h[8] = -1;
    void* dp = nullptr;
    HCK(hipHostGetDevicePointer(&dp, L->h_dc.p, 0));
    L->d_dc = (int*)dp;
}

// The largest shared-entry work of one disk (entries x lower neighbours) a fused poll may report
// before the lane's next polls take the five-launch chain (its union pass spreads crowded shared
// entries over the whole chip; the fused kernel decides a disk's in its own workgroup).
static constexpr int kFwCrowdWork = 2048;

// fp32 entry points (*_f32): every float is widened to the double of the same value (exact), and
// the fp64 path then evaluates the reference predicate on those doubles.
__global__ void widen_f32_kernel(const float* __restrict__ in, int64_t n, double* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = (double)in[t];
}

static void widen_async(const float* d_in, int64_t n, double* d_out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(widen_f32_kernel, dim3(grid1d(n, 256)), dim3(256), 0, s, d_in, n, d_out);
    HCK(hipGetLastError());
}

// host floats -> device doubles through the device scratch `stage`
static void upload_widen(const float* h, int64_t n, DevBuf& stage, double* d_out, hipStream_t s)
{
    if (n <= 0) return;
    stage.reserve(sizeof(float) * (size_t)n);
    HCK(hipMemcpyAsync(stage.p, h, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, s));
    widen_async(stage.as<float>(), n, d_out, s);
}

// mac_profile_kernels' launch roles (include/maxcover.h): the poll chains' own, then the launches
// beside them
static constexpr int kRolePrep = 0, kRoleIndex = 1, kRoleSetup = 2, kRoleTiledPoll = 3, kRolePoll = 4,
                     kRoleShared = 5, kRoleFin = 6, kRoleFiw = 7, kRoleFin2 = 8;
static constexpr int kRoleMask = 9, kRoleProgH = 10, kRoleProgSel = 11;
static_assert(MAC_PROF_ROLES == 12, "the role table");

static inline CandSrc matrix_src(const double* d_cands, int N)
{
    CandSrc c{};
    c.cands = d_cands;
    c.ldc = 3 * N;
    return c;
}

// ------------------------------------------------------------------ point list set-up

static Grid choose_grid(double xmn, double xmx, double ymn, double ymx, int64_t M, int ppt)
{
    Grid g{};
    if (!(xmn <= xmx) || !(ymn <= ymx) || M <= 0) {  // no finite point
        g.gx0 = 0.0;
        g.gy0 = 0.0;
        g.S = 1.0;
        g.invS = 1.0;
        g.nTx = 1;
        g.nTy = 1;
        return g;
    }
    // A finite box whose span overflows counts as DBL_MAX wide: tile_of sends every entry further
    // than that from the origin ((v - g0) = inf) to the last tile, and tile_span's error term
    // overflows with the disk's bound, which gives the whole axis.
    const double W = std::min(xmx - xmn, kDblMax), H = std::min(ymx - ymn, kDblMax);
    // The pitch stays within [2^-1020, 2^1020]: S and 1 / S are both normal doubles, whatever the
    // span (a subnormal W would otherwise give invS = inf, a DBL_MAX one a subnormal invS).
    constexpr double kMinPitch = 0x1p-1020, kMaxPitch = 0x1p1020;
    double S;
    if (W > 0 && H > 0)
        S = std::sqrt(W * H * (double)ppt / (double)M);
    else if (W > 0 || H > 0)
        S = std::max(W, H) * (double)ppt / (double)M;
    else
        S = 1.0;
    if (!(S > 0) || !std::isfinite(S)) S = 1.0;
    S = std::min(std::max(S, kMinPitch), kMaxPitch);
    // cap the tile count (int32 keys, offsets memory): at most max(4M, 2^20) tiles, 2^28 total
    const double cap = std::min(268435456.0, std::max(4.0 * (double)M, 1048576.0));
    for (int it = 0; it < 64; ++it) {
        const double nx = std::floor(W / S) + 1.0, ny = std::floor(H / S) + 1.0;
        if (nx * ny <= cap && nx < 1e8 && ny < 1e8) break;
        S *= 1.5;
    }
    {   // still too many tiles (e.g. a bbox of 1e300 m): at most 1001 x 1001
        const double nx = std::floor(W / S) + 1.0, ny = std::floor(H / S) + 1.0;
        if (!(nx * ny <= cap) || !(nx < 1e8) || !(ny < 1e8)) S = std::max(W, H) / 1000.0;
        S = std::min(std::max(S, kMinPitch), kMaxPitch);
    }
    // The counts come from span * invS (what tile_of computes), the loop's from span / S: where the
    // two round apart at the cap, one more step.
    auto count = [](double span, double inv) { return std::min(std::floor(span * inv) + 1.0, 1e8); };
    while (S < kMaxPitch && count(W, 1.0 / S) * count(H, 1.0 / S) > cap) S = std::min(S * 1.5, kMaxPitch);
    g.gx0 = xmn;
    g.gy0 = ymn;
    g.S = S;
    g.invS = 1.0 / S;
    g.nTx = (int)count(W, g.invS);
    g.nTy = (int)count(H, g.invS);
    if (g.nTx < 1) g.nTx = 1;
    if (g.nTy < 1) g.nTy = 1;
    return g;
}

// Build the tile-sorted copy (xys, ws, perm, off) from ctx->x/y/w (list order), on `s`.
static void build_index(mac_ctx* ctx, hipStream_t s)
{
    const int64_t M = ctx->M;
    // bbox, and whether every entry weighs the same (bit for bit)
    const int nb = (int)std::min<int64_t>(std::max<int64_t>(grid1d(M, kBlock), 1), 1024);
    ctx->bbox.reserve(sizeof(double4) * nb + sizeof(int) * nb);
    int* d_wmix = (int*)(ctx->bbox.as<double4>() + nb);
    hipLaunchKernelGGL(bbox_kernel, dim3(nb), dim3(kBlock), 0, s, ctx->x.as<double>(),
                       ctx->y.as<double>(), ctx->w.as<double>(), M, ctx->bbox.as<double4>(), d_wmix);
    HCK(hipGetLastError());
    std::vector<double4> hb(nb);
    std::vector<int> hw(nb);
    double w0 = 0.0;
    HCK(hipMemcpyAsync(hb.data(), ctx->bbox.p, sizeof(double4) * nb, hipMemcpyDeviceToHost, s));
    HCK(hipMemcpyAsync(hw.data(), d_wmix, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    if (M > 0) HCK(hipMemcpyAsync(&w0, ctx->w.p, sizeof(double), hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    ctx->w_uniform = M > 0;
    for (int v : hw) ctx->w_uniform = ctx->w_uniform && v == 0;
    ctx->w0 = w0;
    double xmn = INFINITY, xmx = -INFINITY, ymn = INFINITY, ymx = -INFINITY;
    for (auto& b : hb) {
        xmn = std::min(xmn, b.x);
        xmx = std::max(xmx, b.y);
        ymn = std::min(ymn, b.z);
        ymx = std::max(ymx, b.w);
    }
    ctx->grid = choose_grid(xmn, xmx, ymn, ymx, M, ctx->tile_ppt);
    ctx->nTiles = (int64_t)ctx->grid.nTx * ctx->grid.nTy;

    ctx->xys.reserve(sizeof(double2) * std::max<int64_t>(M, 1));
    ctx->ws.reserve(sizeof(double) * std::max<int64_t>(M, 1));
    ctx->perm.reserve(sizeof(uint32_t) * std::max<int64_t>(M, 1));
    ctx->off.reserve(sizeof(int32_t) * (ctx->nTiles + 1));
    if (M > 0) {
        ctx->keys_in.reserve(sizeof(uint32_t) * M);
        ctx->keys_out.reserve(sizeof(uint32_t) * M);
        ctx->idx_in.reserve(sizeof(uint32_t) * M);
        hipLaunchKernelGGL(tile_key_kernel, dim3(grid1d(M, 256)), dim3(256), 0, s,
                           ctx->x.as<double>(), ctx->y.as<double>(), M, ctx->grid,
                           ctx->keys_in.as<uint32_t>(), ctx->idx_in.as<uint32_t>());
        HCK(hipGetLastError());
        int end_bit = 1;
        while (end_bit < 32 && ((uint64_t)1 << end_bit) < (uint64_t)ctx->nTiles) ++end_bit;
        size_t tb = 0;
        HCK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ctx->keys_in.as<uint32_t>(),
                                               ctx->keys_out.as<uint32_t>(),
                                               ctx->idx_in.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                                               (int)M, 0, end_bit, s));
        ctx->tmp.reserve(tb);
        HCK(hipcub::DeviceRadixSort::SortPairs(ctx->tmp.p, tb, ctx->keys_in.as<uint32_t>(),
                                               ctx->keys_out.as<uint32_t>(),
                                               ctx->idx_in.as<uint32_t>(), ctx->perm.as<uint32_t>(),
                                               (int)M, 0, end_bit, s));
        hipLaunchKernelGGL(gather_sorted_kernel, dim3(grid1d(M, 256)), dim3(256), 0, s,
                           ctx->x.as<double>(), ctx->y.as<double>(), ctx->w.as<double>(),
                           ctx->perm.as<uint32_t>(), M, ctx->xys.as<double2>(), ctx->ws.as<double>());
        HCK(hipGetLastError());
    }
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(grid1d(ctx->nTiles + 1, 256)), dim3(256), 0, s,
                       ctx->keys_out.as<uint32_t>(), M, ctx->nTiles, ctx->off.as<int32_t>());
    HCK(hipGetLastError());
    HCK(hipStreamSynchronize(s));
    ctx->has_points = true;
}

static int32_t check_M(int64_t M)
{
    if (M < 0) return fail(MAC_E_INVAL, "M < 0");
    if (M >= ((int64_t)1 << 31) - 1) return fail(MAC_E_INVAL, "M must be < 2^31-1");
    return MAC_OK;
}

// ------------------------------------------------------------------ evaluation core

static bool use_tiled(mac_ctx* ctx, int N, const double* h_cands, int64_t three_n)
{
    if (N <= 0 || ctx->algo == MAC_ALGO_SCAN) return false;
    if (ctx->algo == MAC_ALGO_POLL) return true;        // no N limit: fixed LDS footprint
    if (N > kTiledMaxN) return true;                     // the poll walk, whatever K (enqueue_eval)
    if (ctx->algo == MAC_ALGO_TILED) return true;
    if (!h_cands) return true;
    // AUTO with host candidates: compare the tiled walk's point visits for candidate 0 with
    // the scan's M (both per disk); prefer the scan when disks span most of the list.
    const Grid& g = ctx->grid;
    double visits = 0.0;
    for (int i = 0; i < N; ++i) {
        int x0, x1, y0, y1;
        const double r = h_cands[2 * N + i];
        if (!tile_span(h_cands[i], r, g.gx0, g.invS, g.nTx, x0, x1)) continue;
        if (!tile_span(h_cands[N + i], r, g.gy0, g.invS, g.nTy, y0, y1)) continue;
        visits += (double)(x1 - x0 + 1) * (double)(y1 - y0 + 1);
    }
    visits *= (double)ctx->M / (double)std::max<int64_t>(ctx->nTiles, 1);
    (void)three_n;
    return visits < 0.5 * (double)ctx->M * (double)N;
}

// ---- one evaluation

static thread_local std::chrono::steady_clock::time_point t_poll_entry;   // (MAXCOVER_HOST_STATS)

// What the pieces of one enqueue_eval call share: the request and its plan, the buffers of the
// launches ahead of the chains, and the call's profile record.
// Profiling: the measured launches stamp their own workgroups' start / end times (k_common.h), so
// measuring adds no packet, event or dependency to the stream. Each launch takes its slots under
// its role (mac_profile_kernels); the scan and the small-batch walk, outside the chains, under a / na.
struct EvalRun {
    mac_ctx* ctx;
    Lane* L;
    hipStream_t s;
    const EvalReq& rq;
    const EvalPlan& pl;
    double* d_vp = nullptr;             // per-candidate penalty (or +inf: cons3)
    const uint8_t* d_mask8 = nullptr;   // a generated poll's feasibility bytes (mask, prog_h)
    const int* d_mode = nullptr;        // the five-launch chain: the walk the device chose
    mac_ctx::Prof prof{-1, 0, -1, 0, 0, nullptr, 0};

    uint64_t* take_ts(int64_t nwg, int64_t& base, int64_t& n)
    {
        if (!ctx->profile) return nullptr;
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->stamp_used + nwg > ctx->stamp_cap) return nullptr;   // full: not recorded
        base = ctx->stamp_used;
        n = nwg;
        ctx->stamp_used += nwg;
        return ctx->stamps.as<uint64_t>() + 2 * base;
    }
    uint64_t* ts_role(int role, int64_t nwg) { return take_ts(nwg, prof.role[role][0], prof.role[role][1]); }
    uint64_t* ts_lone(int64_t nwg) { return take_ts(nwg, prof.a, prof.na); }
    // (the five-launch chain's inner launches: only when its prep took its stamps)
    uint64_t* ts_chain(int role, int64_t nwg) { return prof.role[kRolePrep][0] >= 0 ? ts_role(role, nwg) : nullptr; }

    // The record of this call: the legacy fields from the roles (a: the walk launch mac_profile_read
    // reads, b: the poll walk beside it, c / f: the chain's first and last launch). A chain whose
    // prep took no stamps (the buffer was full) reports no role of its own.
    void prof_end()
    {
        if (!ctx->profile) return;
        auto& r = prof.role;
        const bool fused = r[kRoleFiw][0] >= 0;
        if (prof.a < 0) {
            prof.a = r[fused ? kRoleFiw : kRoleTiledPoll][0];
            prof.na = r[fused ? kRoleFiw : kRoleTiledPoll][1];
        }
        prof.b = r[kRolePoll][0];
        prof.nb = r[kRolePoll][1];
        if (prof.a < 0 && prof.b < 0) return;
        prof.K = rq.K;
        prof.mode = d_mode;
        prof.algo = fused ? MAC_ALGO_POLL : rq.tiled ? MAC_ALGO_TILED : MAC_ALGO_SCAN;
        prof.c = r[kRolePrep][0];
        prof.nc = r[kRolePrep][1];
        prof.f = r[fused ? kRoleFin2 : kRoleFin][0];
        prof.nf = r[fused ? kRoleFin2 : kRoleFin][1];
        if (prof.c < 0)
            for (int q = 0; q < kRoleMask; ++q) {
                r[q][0] = -1;
                r[q][1] = 0;
            }
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->prof.push_back(prof);
    }
};

// A generated poll of the native MADS driver under swarm constraints: the mask launch first, one
// byte per candidate into the lane's buffer (reused stream-ordered), read by the prep launch. Under
// progressive constraints (mac_mads_run_prog): h of every candidate, and the byte of a candidate the
// barrier drops (h NaN or above h_max) cleared beside the mask's.
static void enqueue_gen_masks(EvalRun& r)
{
    const EvalReq& rq = r.rq;
    const int N = rq.N, K = rq.K;
    r.L->cmask.reserve((size_t)K);
    uint8_t* d_mask = r.L->cmask.as<uint8_t>();
    if (rq.cons) {
        const int S = cons_slots(N);   // (N <= kConsMaxN, checked at begin)
        uint64_t* tsm = r.ts_role(kRoleMask, K);
        if (rq.motion)
            hipLaunchKernelGGL(mask_gen_motion_kern(S, rq.cons->sep), dim3((unsigned)K), dim3(kConsBlock),
                               rq.cons->sep ? mask_lds(S) : 0u, r.s, tsm, rq.src, N, *rq.cons, *rq.motion, d_mask);
        else
            hipLaunchKernelGGL(mask_gen_kern(S), dim3((unsigned)K), dim3(kConsBlock), mask_lds(S), r.s, tsm, rq.src,
                               N, *rq.cons, d_mask);
        HCK(hipGetLastError());
    }
    if (rq.prog) {
        uint64_t* tsp = r.ts_role(kRoleProgH, K);
        hipLaunchKernelGGL(prog_h_kernel, dim3((unsigned)K), dim3(kProgBlock), 0, r.s, tsp, rq.src, N, rq.prog->a,
                           rq.prog->h_max, rq.prog->d_h, d_mask, rq.cons ? 1 : 0);
        HCK(hipGetLastError());
    }
    r.d_mask8 = d_mask;
}

// A generated poll's verdicts (MAC_OPT_VERDICTS; k_cons.h cons_explain_gen_kernel): one launch behind the
// poll's prep launch, so that in the pipelined loop it sees the prep's whole-poll rejection and returns
// as the chain's later launches do. It writes the lane's record scratch and the context's tally; nothing
// of the chain reads either. No profile role, no stamps.
static void enqueue_explain(EvalRun& r)
{
    const EvalReq& rq = r.rq;
    if (!rq.explain || !rq.d_tally || rq.src.cands || rq.K <= 0) return;
    const int N = rq.N, K = rq.K;
    const int S = cons_slots(N);   // (N <= kConsMaxN: mads_begin_check, also under cons3 alone)
    const bool sep = rq.explain->a.sep != 0;
    r.L->verdict.reserve(sizeof(Verdict) * (size_t)K);
    hipLaunchKernelGGL(explain_gen_kern(S, sep), dim3((unsigned)K), dim3(kConsBlock), explain_lds(S, sep), r.s,
                       (uint64_t*)nullptr, rq.src, N, *rq.explain, r.L->verdict.as<Verdict>(), rq.d_tally);
    HCK(hipGetLastError());
}

// The fused chain's turn under AUTO: the lane's last poll's report goes into the context's history,
// and the chain runs unless one of the last 64 reported polls did not suit it: a crowded poll (many
// shared entries: the five-launch chain's union pass), a scattered batch (the per-candidate walk) or
// escaped keys (fp32 keys). Either chain gives the same results. The history is long because a
// wrong choice costs asymmetrically: a crowded poll in the fused chain decides its shared entries
// per candidate in place (0.4-2 ms at configs 5 and 4 clustered), an uncrowded one in the
// five-launch chain costs ~20 us more.
static bool fused_history_allows(mac_ctx* ctx, Lane* L)
{
    ensure_hints(L);
    volatile int* hw = (volatile int*)L->h_dc.p;
    int bad_now = -1;   // the lane's last poll's report (a hint: it may be an older poll's)
    if (L->last_chain == 2 && hw[8] >= 0) {
        bad_now = hw[8] > kFwCrowdWork || hw[9] > 0 || hw[11] > 0 ? 1 : 0;   // (k_fiw.h kFwHints)
        if (ctx->profile) {
            const int64_t id = hw[9];
            ctx->fw_reports.fetch_add(1, std::memory_order_relaxed);
            ctx->fw_ident_sum.fetch_add(id, std::memory_order_relaxed);
            if (id > ctx->fw_ident_max.load(std::memory_order_relaxed))
                ctx->fw_ident_max.store(id, std::memory_order_relaxed);
        }
    }
    else if (L->last_chain == 1 && hw[0] < (1 << 30))
        bad_now = hw[0] > kBitsMinDisks || hw[4] == kModeTiled ? 1 : 0;
    if (bad_now >= 0) {
        uint64_t o = ctx->fused_bad.load(std::memory_order_relaxed);
        while (!ctx->fused_bad.compare_exchange_weak(o, (o << 1) | (uint64_t)bad_now,
                                                     std::memory_order_relaxed)) {
        }
    }
    return ctx->fused_bad.load(std::memory_order_relaxed) == 0;
}

// The key rows of a poll in the lane's buffer: packed keys (one row per disk), then the fp32 rows
// of escaped values (k_prep.h); `src` is the source the launches after the prep read them through.
static void key_rows(Lane* L, int N, int K, PrepArgs& pr, CandSrc& src)
{
    const int ldk = keys_ld(K);
    L->keysT.reserve(sizeof(float) * (size_t)4 * N * ldk);
    pr.keysP = L->keysT.as<uint32_t>();
    pr.keysT = L->keysT.as<float>() + (size_t)N * ldk;
    pr.ldk = ldk;
    src.keysP = pr.keysP;
    src.keysT = pr.keysT;
    src.ldk = ldk;
}

// The prep launch's arguments (k_prep.h: penalty chains + cons3 into vp, the walks' records, the
// index's keys) but the chain's own (prec; xbase, pd, dead8, lreset); nwg: its workgroups.
static PrepArgs prep_args(const EvalRun& r, int nwg, CandSrc& keyed)
{
    const EvalReq& rq = r.rq;
    PrepArgs pr{};
    pr.src = rq.src;
    pr.N = rq.N;
    pr.K = rq.K;
    pr.pa = PenArgs{rq.d_rmax, rq.d_prev, rq.d_dlimT, rq.d_dlim_raw, rq.tan_half_fov};
    pr.penalty = rq.penalty;
    pr.vp = r.d_vp;
    pr.nchain = nwg;
    pr.skip_failed = rq.d_area ? 0 : 1;   // (the index maps them to an inert position likewise)
    pr.pair = r.pl.pair ? 1 : 0;
    pr.g = r.ctx->grid;
    pr.feas = rq.d_feas;
    pr.mask8 = r.d_mask8;
    // the pipelined MADS loop: a poll cons3 rejects whole is decided by the prep (k_prep.h
    // MadsState.skip) when its failures are left out of the walk
    pr.mst_w = rq.fb_mads && r.pl.poll_possible && r.pl.excl && rq.d_prev ? rq.fb_mads->st : nullptr;
    if (r.pl.want_keys) key_rows(r.L, rq.N, rq.K, pr, keyed);
    return pr;
}

// The argmin's arguments of the chain's last launch (k_final.h: taken by its last-arriving block of
// nfin); all zero without d_best.
static FinBest fin_best(const EvalRun& r, unsigned nfin)
{
    const EvalReq& rq = r.rq;
    Lane* L = r.L;
    FinBest fb{};
    if (!rq.d_best) return fb;
    L->finblk.reserve(2 * sizeof(unsigned long long) * nfin);
    // (8 shard words and a root, a line each) zero once; the reducer of each launch resets them
    if (L->finarrive.grow(sizeof(unsigned) * kFinArriveWords))
        HCK(hipMemsetAsync(L->finarrive.p, 0, L->finarrive.cap, r.s));
    if (rq.fb_mads) fb = *rq.fb_mads;   // the pipelined MADS loop's update fields
    fb.best = rq.d_best;
    fb.mirror = rq.d_mirror;
    fb.seq = rq.mirror_seq;
    fb.idx_base = rq.idx_base;
    fb.blk = L->finblk.as<unsigned long long>();
    fb.arrive = L->finarrive.as<unsigned>();
    fb.feas = rq.d_mirror ? rq.d_feas : nullptr;
    return fb;
}

// The fused chain (k_fiw.h): prep -> fiw_kernel -> fin2_kernel.
static void enqueue_fused(EvalRun& r)
{
    const EvalReq& rq = r.rq;
    const EvalPlan& pl = r.pl;
    mac_ctx* ctx = r.ctx;
    Lane* L = r.L;
    hipStream_t s = r.s;
    const int N = rq.N, K = rq.K, counts = pl.counts;
    const bool mat = rq.src.cands != nullptr;
    FwArgs fa{};
    fa.src = rq.src;
    PrepArgs pr = prep_args(r, pl.nprep, fa.src);
    const int ldk = pr.ldk;
    L->pd.reserve(sizeof(double4) * (size_t)pl.nprep);
    L->frows.reserve((counts ? sizeof(unsigned) : sizeof(double)) * (size_t)N * ldk);
    if (L->fwhint.grow(sizeof(int) * kFwHints)) HCK(hipMemsetAsync(L->fwhint.p, 0, L->fwhint.cap, s));
    if (pl.excl) L->dead8.reserve((size_t)ldk + 16);   // (the fused kernel reads 4-B words)
    L->fwlist.reserve(sizeof(int4) * (size_t)std::max(N, kF2Pre));
    if (L->fwcount.grow(sizeof(int))) HCK(hipMemsetAsync(L->fwcount.p, 0, L->fwcount.cap, s));
    L->fwsxy.reserve(sizeof(double2) * (size_t)N * kFwShCap);
    L->fwsw.reserve(sizeof(double) * (size_t)N * kFwShCap);
    pr.xbase = pl.xbase;
    pr.pd = L->pd.as<double4>();
    pr.dead8 = pl.excl ? L->dead8.as<uint8_t>() : nullptr;
    pr.lreset = L->fwcount.as<int>();
    uint64_t* tsk = r.ts_role(kRolePrep, pl.nprep);
    using hclk = std::chrono::steady_clock;
    hclk::time_point h1, h2, h3;
    if (ctx->host_stats) h1 = hclk::now();
    hipLaunchKernelGGL(prep_kern(pl.prep_fused, pl.mesh), dim3((unsigned)pl.nprep), prep_block(pl.prep_fused), 0, s,
                       tsk, pr);
    HCK(hipGetLastError());
    enqueue_explain(r);
    if (ctx->host_stats) h2 = hclk::now();
    fa.N = N;
    fa.K = K;
    fa.g = ctx->grid;
    fa.dead = pr.dead8;
    fa.pd = pr.pd;
    fa.npd = pl.nprep;
    fa.xy = ctx->xys.as<double2>();
    fa.w = ctx->ws.as<double>();
    fa.off = ctx->off.as<int32_t>();
    fa.counts = counts;
    fa.crow = L->frows.as<unsigned>();
    fa.frow = L->frows.as<double>();
    fa.ldk = ldk;
    fa.hint = L->fwhint.as<int>();
    fa.sh = FwShared{L->fwcount.as<int>(), L->fwlist.as<int4>(), L->fwsxy.as<double2>(), L->fwsw.as<double>()};
    const F2Shared f2s{fa.src, L->fwcount.as<int>(), L->fwlist.as<int4>(), L->fwsxy.as<double2>(),
                       L->fwsw.as<double>(), fa.dead};
    uint64_t* tsw = r.ts_role(kRoleFiw, pl.nfw);
    hipLaunchKernelGGL(fiw_kern(counts, mat, pl.mesh), dim3(pl.nfw), dim3(kFwThreads), 0, s, tsw, fa);
    HCK(hipGetLastError());
    if (ctx->host_stats) h3 = hclk::now();
    FinBest fb = fin_best(r, pl.nfin2);
    if (rq.d_best) {
        fb.hint = L->fwhint.as<int>();   // (read and cleared by the argmin's last block)
        fb.hint_host = L->d_dc + 8;
        fb.nhint = kFwHints;
    }
    uint64_t* tsf = r.ts_role(kRoleFin2, pl.nfin2);
    // (fb.np: the pipelined loop's update of an xy-only poll, a generated source)
    hipLaunchKernelGGL(fin2_kern(counts, mat, fb.np != 0, pl.mesh), dim3(pl.nfin2), dim3(kF2Threads), 0, s,
                       counts ? L->frows.as<unsigned>() : nullptr, counts ? nullptr : L->frows.as<double>(),
                       ldk, N, K, ctx->w0, r.d_vp, rq.d_area, rq.d_obj, fb, f2s, tsf);
    HCK(hipGetLastError());
    if (ctx->host_stats) {
        const auto h4 = hclk::now();
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->hs_t[0] += std::chrono::duration<double>(h1 - t_poll_entry).count();
        ctx->hs_t[1] += std::chrono::duration<double>(h2 - h1).count();
        ctx->hs_t[2] += std::chrono::duration<double>(h3 - h2).count();
        ctx->hs_t[3] += std::chrono::duration<double>(h4 - h3).count();
        ++ctx->hs_n;
    }
    L->last_chain = 2;
}

// What the walks hand to finalize_kernel (k_final.h).
struct WalkOut {
    int n_other = 1;                   // partial rows per candidate of the scan / per-candidate walk
    const int* d_umap = nullptr;       // poll walk: candidate -> distinct-disk position
    const double* d_spart = nullptr;   // poll walk: shared-entry rows
    const int* d_ncount = nullptr;
};

// The streaming scan: every entry against every candidate's disks.
static void enqueue_scan(EvalRun& r, WalkOut& w)
{
    mac_ctx* ctx = r.ctx;
    Lane* L = r.L;
    const int N = r.rq.N, K = r.rq.K;
    const int64_t M = ctx->M;
    L->disks.reserve(sizeof(DiskRec) * (size_t)N * K);
    hipLaunchKernelGGL(disk_prep_kernel, dim3(grid1d((int64_t)N * K, 256)), dim3(256), 0, r.s, r.rq.src, N, K,
                       L->disks.as<DiskRec>());
    HCK(hipGetLastError());
    constexpr int KB = 4, PPT = 4;
    const int64_t per_pass = (int64_t)kBlock * PPT;
    int64_t nblk = std::max<int64_t>(1, (M + per_pass - 1) / per_pass);
    const int kgroups = (K + KB - 1) / KB;
    const int64_t want = std::max<int64_t>(1, (int64_t)(8 * ctx->cus) / kgroups);
    nblk = std::min(nblk, want);
    int64_t chunk = (M + nblk - 1) / nblk;
    chunk = ((chunk + per_pass - 1) / per_pass) * per_pass;
    nblk = std::max<int64_t>(1, (M + chunk - 1) / chunk);
    w.n_other = (int)nblk;
    L->partial.reserve(sizeof(double) * (size_t)K * nblk);
    uint64_t* ts = r.ts_lone(nblk * kgroups);
    hipLaunchKernelGGL((coverage_scan_kernel<KB, PPT>), dim3((unsigned)nblk, (unsigned)kgroups), dim3(kBlock), 0,
                       r.s, ts, ctx->xys.as<double2>(), ctx->ws.as<double>(), M, L->disks.as<DiskRec>(), N, K, chunk,
                       L->partial.as<double>());
    HCK(hipGetLastError());
}

// The per-candidate walk alone (small batches, the single-candidate closure): the identity map, one
// thread per (disk, candidate), no key pass.
static void enqueue_small_walk(EvalRun& r, WalkOut& w)
{
    mac_ctx* ctx = r.ctx;
    Lane* L = r.L;
    const int N = r.rq.N, K = r.rq.K, G = r.pl.G;
    L->disks.reserve(sizeof(DiskRec) * (size_t)N * K);
    L->umap.reserve(sizeof(int) * (size_t)N * K);
    L->ucount.reserve(sizeof(int) * (size_t)N);
    w.n_other = G;
    hipLaunchKernelGGL(disk_index_identity_kernel, dim3(grid1d((int64_t)N * K, 256)), dim3(256), 0, r.s, r.rq.src,
                       N, K, L->disks.as<DiskRec>(), L->umap.as<int>());
    HCK(hipGetLastError());
    L->partial.reserve(sizeof(double) * (size_t)K * G);
    uint64_t* ts = r.ts_lone(r.pl.units);
    hipLaunchKernelGGL(coverage_tiled_kernel, dim3((unsigned)r.pl.units), dim3(kBlock), (uint32_t)tiled_lds_bytes(N),
                       r.s, ts, ctx->xys.as<double2>(), ctx->ws.as<double>(), ctx->off.as<int32_t>(), ctx->grid,
                       L->disks.as<DiskRec>(), L->umap.as<int>(), N, K, G, nullptr, L->partial.as<double>());
    HCK(hipGetLastError());
}

// The prep launch of the five-launch chain, and of an evaluation without a chain that wants
// objectives (the penalties alone). `keyed`: the source the index reads the keys through.
static void enqueue_prep_five(EvalRun& r, CandSrc& keyed)
{
    const EvalPlan& pl = r.pl;
    PrepArgs pr = prep_args(r, pl.nrec, keyed);
    if (pl.poll_possible) {
        r.L->prec.reserve(sizeof(int4) * (size_t)pl.nrec * r.rq.N);
        pr.prec = r.L->prec.as<int4>();
    }
    uint64_t* tsk = pl.poll_possible ? r.ts_role(kRolePrep, pl.nrec) : nullptr;
    hipLaunchKernelGGL(prep_kern(pl.prep_five, pl.mesh), dim3((unsigned)pl.nrec), prep_block(pl.prep_five), 0, r.s,
                       tsk, pr);
    HCK(hipGetLastError());
    enqueue_explain(r);
}

// The shared entries of crowded polls: the union pass (equal weights, k_or.h) or bit-words per
// distinct position (k_bits.h); both return at once when few disks have neighbours (the poll
// kernel took them).
static void enqueue_shared_pass(EvalRun& r, int bits_on)
{
    mac_ctx* ctx = r.ctx;
    Lane* L = r.L;
    const int N = r.rq.N, K = r.rq.K;
    const DiskRec* d_urec = L->disks.as<DiskRec>();
    const int* d_map = L->umap.as<int>();
    const unsigned nbits = (unsigned)std::max(1, std::min(N, ctx->cus));
    const unsigned nor = (unsigned)(2 * ctx->cus);   // grid-strides over the listed jobs
    uint64_t* tsg = r.ts_chain(kRoleShared, r.pl.counts ? nor : nbits);
    if (r.pl.counts) {
        OrArgs oa{};
        oa.xy = ctx->xys.as<double2>();
        oa.off = ctx->off.as<int32_t>();
        oa.g = ctx->grid;
        oa.urec = d_urec;
        oa.umap = d_map;
        oa.ucount = L->ucount.as<int>();
        oa.region = L->region.as<int4>();
        oa.nbrT = L->nbr.as<uint16_t>();
        oa.nboxT = L->nboxT.as<int4>();
        oa.ncount = L->ncount.as<int>();
        oa.nboxU = L->nboxU.as<int4>();
        oa.ncountU = L->ncountU.as<int>();
        oa.lane4 = L->lane4.as<float4>();
        oa.lanexp = L->lanexp.as<float>();
        oa.jobs = L->orjobs.as<int2>();
        oa.dcount = L->mode.as<int>() + 1;
        oa.mode = r.d_mode;
        oa.spart = L->spart.as<unsigned>();
        oa.N = N;
        oa.K = K;
        oa.bits_on = bits_on;
        oa.cap = (int)(ctx->M / kOrE + N + 64);
        hipLaunchKernelGGL(shared_or_kernel, dim3(nor), dim3(kOrThreads), 0, r.s, tsg, oa);
    } else
        hipLaunchKernelGGL(shared_bits_kernel<false>, dim3(nbits), dim3(kBitsThreads), 0, r.s, tsg,
                           ctx->xys.as<double2>(), ctx->ws.as<double>(), ctx->off.as<int32_t>(), ctx->grid, d_urec,
                           d_map, L->ucount.as<int>(), L->region.as<int4>(), L->nbr.as<uint16_t>(),
                           L->lane4.as<float4>(), L->lanexp.as<float>(), L->ncount.as<int>(), L->qual.as<int>(),
                           L->mode.as<int>() + 1, r.d_mode, N, K, L->spart.as<double>(),
                           bits_on == 2 ? 0 : kBitsMinDisks);
    HCK(hipGetLastError());
}

// The shared-entry pass's launch hint (the walk set-up, the poll walk and the pass itself read it):
// 0: fp64 jobs; 1: above kBitsMinDisks disks with neighbours; 2: always. Launched when one of the
// lane's last 8 polls had more than kBitsMinDisks disks with neighbours (the poll kernel writes the
// count to mapped host memory): a hint only, the poll kernel takes every disk when it is not
// launched (MADS alternates crowded and quiet polls, and a crowded poll without the pass costs
// several times its launch).
static int shared_pass_hint(mac_ctx* ctx, Lane* L)
{
    const int dc_now = *(volatile int*)L->h_dc.p;   // 1 << 30 until a poll wrote it
    int dc_max = dc_now;
    if (dc_now < (1 << 30)) {
        for (int q = 7; q > 0; --q) L->dc_hist[q] = L->dc_hist[q - 1];
        L->dc_hist[0] = dc_now;
        for (int q = 0; q < 8; ++q) dc_max = std::max(dc_max, L->dc_hist[q]);
    }
    int bits_on = ctx->shared_mode == MAC_SHARED_BITS ? 2
                : ctx->shared_mode == MAC_SHARED_FP64 ? 0
                : dc_max > kBitsMinDisks ? 1 : 0;
    // Both passes stage an entry as its fp32 offset (u, v) from a region's centre with
    // q = u u + v v, and q = +inf marks "no entry" (k_or.h, k_bits.h: outside the box, past
    // the list, non-finite). A finite entry must therefore keep q finite: |u|, |v| below
    // 2^63. Offsets are bounded by the grid's extent, so on a grid of 2^62 or more (a far
    // outlier sets the pitch: the centre of the tile that holds the rest of the list lies
    // S / 2 away from it) finite entries would drop out of the unions, and the poll
    // kernel's fp64 jobs take every disk there.
    const Grid& gr = ctx->grid;
    if (!(((double)std::max(gr.nTx, gr.nTy) + 1.0) * gr.S < 0x1p62)) bits_on = 0;
    return bits_on;
}

// The five-launch chain after its prep: the disk index (distinct disks per UAV, their records, the
// map and the poll walk's lane constants, k_index.h), the walk set-up, the walks and the shared pass.
// `keyed`: the source with the prep's key rows.
static void enqueue_five(EvalRun& r, const CandSrc& keyed, WalkOut& w)
{
    const EvalReq& rq = r.rq;
    const EvalPlan& pl = r.pl;
    mac_ctx* ctx = r.ctx;
    Lane* L = r.L;
    hipStream_t s = r.s;
    const int N = rq.N, K = rq.K, G = pl.G, counts = pl.counts;
    L->disks.reserve(sizeof(DiskRec) * (size_t)N * K);
    L->umap.reserve(sizeof(int) * (size_t)N * K);
    L->ucount.reserve(sizeof(int) * (size_t)N);
    // the poll walk's lane constants and row descriptors
    L->lane4.reserve(sizeof(float4) * (size_t)N * K);
    L->lanexp.reserve(sizeof(float) * (size_t)N * K);
    L->rows.reserve(sizeof(int2) * (size_t)N * (kRowInfo + 1));
    w.n_other = G;
    const DiskRec* d_urec = L->disks.as<DiskRec>();
    const int* d_map = L->umap.as<int>();
    L->region.reserve(sizeof(int4) * N);
    L->cost.reserve(sizeof(double2) * N);
    L->mode.reserve((1 + kDcCount) * sizeof(int));  // [0] walk, [1..kDcCount] the poll walk's counters (k_common.h)
    const IndexOut io{L->disks.as<DiskRec>(), L->umap.as<int>(), L->ucount.as<int>(),
                      L->region.as<int4>(), L->cost.as<double2>(), L->mode.as<int>() + 1,
                      L->prec.as<int4>(), pl.nrec,
                      L->lane4.as<float4>(), L->lanexp.as<float>(), L->rows.as<int2>(),
                      ctx->off.as<int32_t>(),
                      // cons3 failures are not evaluated (objective +inf) unless the caller
                      // also wants every candidate's area
                      rq.d_area ? nullptr : r.d_vp};
    uint64_t* tsi = r.ts_chain(kRoleIndex, pl.nidx);
    hipLaunchKernelGGL(index_kern(keyed.keysT != nullptr, pl.iper == kIdxPerWide, keyed.np != 0, pl.mesh),
                       dim3(pl.nidx), dim3(kIdxThreads), 0, s, tsi, keyed, N, K, ctx->grid, pl.iper ? 1 : 0, io);
    HCK(hipGetLastError());
    // launch hints from the lane's previous polls (mapped host memory the poll kernel
    // writes): disks with neighbours, most positions of a disk, the walk AUTO would choose
    ensure_hints(L);
    // neighbour lists (k_walk.h walk_setup_kernel), then — when the per-candidate walk is
    // forced, or AUTO chose it on one of the lane's last 8 polls — the walk choice and that
    // walk (coverage_tiled_poll_kernel). Otherwise the poll walk runs; its kernel records
    // the choice AUTO would have made, so a batch that favours the per-candidate walk gets
    // it from the lane's next poll on (the choice only changes speed, never results).
    // (a lane's first poll has no report yet: it launches the kernel once, and the
    // sentinel stays out of the history)
    const int walk_now = ((volatile int*)L->h_dc.p)[4];
    bool hinted = walk_now == 0;
    if (!hinted) {
        for (int q = 7; q > 0; --q) L->walk_hist[q] = L->walk_hist[q - 1];
        L->walk_hist[0] = walk_now;
    }
    for (int q = 0; q < 8; ++q) hinted |= L->walk_hist[q] == kModeTiled;
    const bool run_tiled = pl.walk_forced == kModeTiled || (pl.walk_forced == 0 && hinted);
    L->nbr.reserve(sizeof(uint16_t) * (size_t)N * kPollNbr);
    L->ncount.reserve(sizeof(int) * (size_t)N);
    L->dlist.reserve(sizeof(int) * (size_t)N);
    L->qual.reserve(sizeof(int) * (size_t)N);
    L->nboxT.reserve(sizeof(int4) * (size_t)N * kPollNbr);
    L->partial.reserve(sizeof(double) * (size_t)K * std::max(G, N));
    const int bits_on = shared_pass_hint(ctx, L);
    // equal weights: the union pass (k_or.h), whose jobs walk_setup lists with the upper
    // neighbour boxes; weighted lists: the bit-word kernel (k_bits.h)
    OrSetup orj{};
    if (bits_on && counts) {
        L->nboxU.reserve(sizeof(int4) * (size_t)N * kPollNbr);
        L->ncountU.reserve(sizeof(int) * (size_t)N);
        const int64_t cap = ctx->M / kOrE + N + 64;   // the owned sets are disjoint
        L->orjobs.reserve(sizeof(int2) * (size_t)cap * kOrBuckets);   // a list per bucket
        orj = OrSetup{L->nboxU.as<int4>(), L->ncountU.as<int>(), L->orjobs.as<int2>(), (int)cap,
                      ctx->off.as<int32_t>(), ctx->grid, L->ucount.as<int>()};
    }
    uint64_t* tss = r.ts_chain(kRoleSetup, N);
    hipLaunchKernelGGL(walk_setup_kernel, dim3((unsigned)N), dim3(kBlock), 0, s, tss, N,
                       L->region.as<int4>(), L->nbr.as<uint16_t>(), L->nboxT.as<int4>(),
                       L->ncount.as<int>(), L->dlist.as<int>(), L->mode.as<int>() + 1,
                       L->mode.as<int>(), L->qual.as<int>(), rq.src.mst, orj);
    HCK(hipGetLastError());
    if (run_tiled) {
        // one workgroup per CU at most, grid-striding over the (candidate, slice) units
        const unsigned nwg = (unsigned)std::max<int64_t>(1, std::min<int64_t>(pl.units, ctx->cus));
        uint64_t* ts = r.ts_role(kRoleTiledPoll, nwg);
        hipLaunchKernelGGL(coverage_tiled_poll_kernel, dim3(nwg), dim3(kBlock),
                           (uint32_t)tiled_lds_bytes(N), s, ts, ctx->xys.as<double2>(),
                           ctx->ws.as<double>(), ctx->off.as<int32_t>(), ctx->grid, d_urec, d_map,
                           N, K, G, L->mode.as<int>(), L->partial.as<double>(),
                           L->nbr.as<uint16_t>(), L->ncount.as<int>(), L->cost.as<double2>(),
                           kPollCostRatio, pl.walk_forced, L->d_dc + 4);
        HCK(hipGetLastError());
    }
    r.d_mode = L->mode.as<int>();
    w.d_umap = d_map;
    // walk rows: the lane's last 8 polls' most distinct positions of a disk (poll kernel
    // hint), one row per kPollKPB-position slice up to 4 (further slices loop)
    const int um_now = ((volatile int*)L->h_dc.p)[2];
    for (int q = 7; q > 0; --q) L->um_hist[q] = L->um_hist[q - 1];
    L->um_hist[0] = um_now;
    int um_max = 0;
    for (int q = 0; q < 8; ++q) um_max = std::max(um_max, L->um_hist[q]);
    const int gy = std::max(1, std::min(4, (um_max + kPollKPB - 1) / kPollKPB));
    L->spart.reserve(sizeof(double) * (size_t)N * K);
    const int n_shared = kSharedWG;
    const dim3 pgrid(pl.nidx + n_shared, gy);   // walk workgroups (8 per disk group), then shared
    uint64_t* ts = r.ts_role(kRolePoll, (int64_t)pgrid.x * pgrid.y);
    hipLaunchKernelGGL(coverage_poll_kernel, pgrid, dim3(kPollThreads), 0, s, ts,
                       ctx->xys.as<double2>(), ctx->ws.as<double>(),
                       ctx->off.as<int32_t>(), ctx->grid, d_urec, d_map,
                       L->ucount.as<int>(), L->region.as<int4>(), L->nbr.as<uint16_t>(),
                       L->nboxT.as<int4>(), L->lane4.as<float4>(), L->lanexp.as<float>(),
                       L->rows.as<int2>(),
                       L->ncount.as<int>(), L->dlist.as<int>(), L->mode.as<int>() + 1,
                       L->mode.as<int>() + 2, N, K,
                       r.d_mode, L->partial.as<double>(), L->spart.as<double>(), n_shared, counts,
                       bits_on, L->d_dc, L->qual.as<int>(),
                       pl.walk_forced == 0 ? L->cost.as<double2>() : nullptr, kPollCostRatio);
    HCK(hipGetLastError());
    if (bits_on) enqueue_shared_pass(r, bits_on);
    ctx->last_five.store(L, std::memory_order_relaxed);
    w.d_spart = L->spart.as<double>();
    w.d_ncount = L->ncount.as<int>();
}

// finalize_kernel, with the poll argmin taken by its last-arriving block (k_final.h).
static void enqueue_finalize(EvalRun& r, const WalkOut& w)
{
    const EvalReq& rq = r.rq;
    const EvalPlan& pl = r.pl;
    const FinBest fb = fin_best(r, pl.nfin);
    uint64_t* tsf = r.ts_chain(kRoleFin, pl.nfin);
    // (fb.np: the pipelined loop's update of an xy-only poll)
    // (... and on a mesh: the builds with the scaled update; a stepper's finalize applies none)
    hipLaunchKernelGGL(finalize_kern(fb.np != 0, pl.mesh != 0 && fb.st != nullptr), dim3(pl.nfin), dim3(kFinThreads), 0,
                       r.s, r.L->partial.as<double>(), r.d_mode, rq.N, w.n_other, rq.K, rq.N, w.d_umap, w.d_spart,
                       w.d_ncount, pl.counts, r.ctx->w0, r.d_vp, rq.d_area, rq.d_obj, fb, tsf);
    HCK(hipGetLastError());
}

// What eval_plan reads of a request on this context (mask: a feasibility byte per candidate).
static RouteIn route_in(const mac_ctx* ctx, const EvalReq& rq, bool mask)
{
    const CandSrc& src = rq.src;
    RouteIn in;
    in.algo = ctx->algo;
    in.chain = ctx->chain;
    in.cus = ctx->cus;
    in.M = ctx->M;
    in.w_uniform = ctx->w_uniform;
    in.kind = src.cands ? RouteIn::kMatrix : src.ltri ? RouteIn::kBasis : RouteIn::kGenerated;
    in.np = src.np;
    in.k0 = src.k0;
    in.mesh = src.mesh() != nullptr;
    in.mst = src.mst != nullptr;
    in.route_five = src.route_five != 0;
    in.mesh_keys = src.mesh_keys != 0;
    in.b = src.b;
    in.delta = src.delta;
    in.want_area = rq.d_area != nullptr;
    in.want_obj = rq.d_obj != nullptr;
    in.cons3 = rq.d_prev != nullptr;
    in.mask = mask;
    in.tiled = rq.tiled;
    in.N = rq.N;
    in.K = rq.K;
    return in;
}

// Enqueue one evaluation on stream s: the route (eval_plan), a generated poll's mask launches, then
// the fused chain, or the prep launch + index + walks + finalize (+ argmin).
static void enqueue_eval(mac_ctx* ctx, Lane* L, hipStream_t s, const EvalReq& rq)
{
    const int K = rq.K;
    const bool gen_masks = (rq.cons || rq.prog) && !rq.src.cands && rq.d_obj && K > 0;
    const EvalPlan pl = eval_plan(route_in(ctx, rq, gen_masks));
    EvalRun r{ctx, L, s, rq, pl};
    if (rq.d_obj) {
        L->vp.reserve(sizeof(double) * (size_t)std::max(K, 1));
        r.d_vp = L->vp.as<double>();
    }
    if (gen_masks) enqueue_gen_masks(r);
    // the history is read and updated at every eligible poll, also one whose chain is forced
    if (pl.fused_eligible && (fused_history_allows(ctx, L) || ctx->chain == MAC_CHAIN_FUSED)) {
        enqueue_fused(r);
        r.prof_end();
        return;
    }
    if (pl.poll_possible) L->last_chain = 1;
    CandSrc keyed = rq.src;
    if (pl.prep_five_runs) enqueue_prep_five(r, keyed);
    WalkOut w;
    if (rq.N == 0 || ctx->M == 0) {  // no UAV or no entry: every area is 0 (the loops never run)
        L->partial.reserve(sizeof(double) * (size_t)K);
        HCK(hipMemsetAsync(L->partial.p, 0, sizeof(double) * (size_t)K, s));
    } else if (!rq.tiled)
        enqueue_scan(r, w);
    else if (!pl.poll_possible)
        enqueue_small_walk(r, w);
    else
        enqueue_five(r, keyed, w);
    enqueue_finalize(r, w);
    r.prof_end();
}

static double dlim_threshold(double d) { return mac::dlim_threshold(d); }

// cons3's inputs into the lane, on s: prev (3N) into L->prev, d_lim thresholded per UAV into L->dlim
// (on the host: L->h_dlim) and as it is into L->dlimraw.
template <class T>
static void cons3_upload(Lane* L, hipStream_t s, int N, const T* prev, const double* d_lim)
{
    const int64_t three_n = 3 * (int64_t)N;
    L->prev.reserve(sizeof(double) * three_n);
    L->dlim.reserve(sizeof(double) * N);
    L->dlimraw.reserve(sizeof(double) * N);
    L->h_dlim.resize(N);
    for (int i = 0; i < N; ++i) L->h_dlim[i] = dlim_threshold(d_lim[i]);
    if constexpr (std::is_same<T, float>::value)
        upload_widen(prev, three_n, L->p32, L->prev.as<double>(), s);
    else
        HCK(hipMemcpyAsync(L->prev.p, prev, sizeof(double) * three_n, hipMemcpyHostToDevice, s));
    HCK(hipMemcpyAsync(L->dlim.p, L->h_dlim.data(), sizeof(double) * N, hipMemcpyHostToDevice, s));
    HCK(hipMemcpyAsync(L->dlimraw.p, d_lim, sizeof(double) * N, hipMemcpyHostToDevice, s));
}

static int32_t check_common(mac_ctx* ctx, int64_t three_n, int64_t K)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (three_n < 0 || K < 0) return fail(MAC_E_INVAL, "negative size");
    if (three_n % 3 != 0)
        return fail(MAC_E_SIZE, "InexactError: Int64(" + std::to_string(three_n) + "/3)");
    if (!ctx->has_points) return fail(MAC_E_NOPOINTS, "no point list set");
    if (three_n / 3 > 65535) return fail(MAC_E_INVAL, "N > 65535 UAVs");
    if (K > (int64_t)1 << 30) return fail(MAC_E_INVAL, "K too large");
    return MAC_OK;
}

// Host-pointer batch: upload, evaluate, download.

// Routing a generated poll from the poll itself (the native MADS driver knows its incumbent and mesh
// step): the fused chain's superset boxes (k_fiw.h sup_box: every candidate's disk i lies within b of
// the incumbent's per coordinate, so box i is within 2b + r_i of its centre, plus a tile of
// rounding) overlap-tested by a sweep over the boxes sorted by their x start. More than
// kBitsMinDisks disks with a lower-index neighbour is a crowded poll (the five-launch chain's
// union pass decides its shared entries once; the fused chain would decide them per candidate in
// place, 5-20x slower: tools/c5_route.py). Returns that count.
static int host_crowded_disks(const double* x, int N, double b, double S)
{
    struct Bx {
        double x0, x1, y0, y1;
        int i;
    };
    std::vector<Bx> v;
    v.reserve(N);
    for (int i = 0; i < N; ++i) {
        const double r = x[2 * N + i];
        if (!(r + b > 0.0)) continue;   // covers nothing at any candidate
        const double h = 2.0 * b + std::fabs(r) + S;
        if (!std::isfinite(h) || !std::isfinite(x[i]) || !std::isfinite(x[N + i])) return N;   // (unknown)
        v.push_back({x[i] - h, x[i] + h, x[N + i] - h, x[N + i] + h, i});
    }
    std::sort(v.begin(), v.end(), [](const Bx& a, const Bx& c) { return a.x0 < c.x0; });
    std::vector<char> has(N, 0);
    std::vector<int> act;   // boxes whose x range may still reach later starts
    for (int q = 0; q < (int)v.size(); ++q) {
        const Bx& c = v[q];
        int w = 0;
        for (int a : act) {
            const Bx& o = v[a];
            if (o.x1 < c.x0) continue;   // (dropped: no later box starts before it ends)
            act[w++] = a;
            if (o.y0 <= c.y1 && c.y0 <= o.y1) has[std::max(o.i, c.i)] = 1;
        }
        act.resize(w);
        act.push_back(q);
    }
    int n = 0;
    for (char h : has) n += h;
    return n;
}

// A context's first matrix poll routes from the poll, before any chain has reported to the history
// above: its candidate 0 (a DirectSearch poll's incumbent) overlap-tested as host_crowded_disks
// does for generated polls, with no displacement (the matrix's spread is unknown here). A crowded
// incumbent starts the history all "unsuited" (the five-launch chain; the fused chain again after
// 64 polls that suit it), so a crowded poll does not pay the fused chain's in-place shared
// decisions on its first call (clustered config 4: 2.7 ms against 0.17). Not from an arming call
// (its stream waits on the doorbell: no synchronous copy there).
static void seed_route(mac_ctx* ctx, const double* x0, int N)
{
    if (N > 0 && host_crowded_disks(x0, N, 0.0, ctx->grid.S) > kBitsMinDisks)
        ctx->fused_bad.store(~(uint64_t)0, std::memory_order_relaxed);
}

// A large host buffer into device memory through the lane's pinned staging: host threads copy
// chunks into the staging while this thread enqueues each chunk's async copy as soon as it has
// landed (a single-threaded memcpy of config 4's 37.7-MB matrix took ~3 ms before the first byte
// moved; MAXCOVER_STAGE_THREADS sets the threads, 1 = the plain copy). Returns once every copy is
// enqueued and every host thread has finished (the staging may then be reused after the stream).
static const int kStageThreads = [] {
    const char* e = std::getenv("MAXCOVER_STAGE_THREADS");
    const int v = e ? std::atoi(e) : 8;
    return std::max(1, std::min(v, 32));
}();

static void staged_upload(const void* src, void* pinned, void* dev, size_t bytes, hipStream_t s)
{
    constexpr size_t kChunk = (size_t)4 << 20;
    const int T = (int)std::min<size_t>((size_t)kStageThreads, (bytes + kChunk - 1) / kChunk);
    if (T <= 1 || bytes < 2 * kChunk) {
        std::memcpy(pinned, src, bytes);
        HCK(hipMemcpyAsync(dev, pinned, bytes, hipMemcpyHostToDevice, s));
        return;
    }
    const size_t nc = (bytes + kChunk - 1) / kChunk;
    std::vector<std::atomic<int>> done(nc);
    for (auto& d : done) d.store(0, std::memory_order_relaxed);
    auto work = [&](int t) {   // chunks t, t + T, ...: the early chunks land first
        for (size_t c = (size_t)t; c < nc; c += (size_t)T) {
            const size_t o = c * kChunk, n = std::min(kChunk, bytes - o);
            std::memcpy((char*)pinned + o, (const char*)src + o, n);
            done[c].store(1, std::memory_order_release);
        }
    };
    std::vector<std::thread> th;
    int started = 1;   // workers 1 .. started-1 run on their own threads; the rest on this one
    try {
        th.reserve((size_t)T - 1);
        for (int t = 1; t < T; ++t, ++started) th.emplace_back(work, t);
    } catch (...) {   // (no thread to spare: this thread copies their chunks too)
    }
    for (int t = started; t < T; ++t) work(t);
    work(0);
    HipError err{hipSuccess, "", 0};
    for (size_t c = 0; c < nc; ++c) {   // (every thread is joined before an error leaves)
        while (!done[c].load(std::memory_order_acquire)) std::this_thread::yield();
        const size_t o = c * kChunk, n = std::min(kChunk, bytes - o);
        if (err.e == hipSuccess) {
            const hipError_t e = hipMemcpyAsync((char*)dev + o, (const char*)pinned + o, n, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) err = HipError{e, "hipMemcpyAsync (staged_upload)", __LINE__};
        }
    }
    for (auto& t : th) t.join();
    if (err.e != hipSuccess) throw err;
}

// ---- swarm constraints (k_cons.h): the mask launch and the masked poll's argmin

// The kernel's arguments from a mac_cons; false when every constraint is off (or cons is null).
static bool cons_active(const mac_cons* cons, ConsArgs* a)
{
    if (!cons) return false;
    *a = cons_args(cons->d_sep, cons->zone_y, cons->zone_r);
    return a->sep || a->zone;
}

// Which motion constraints of a mac_motion are on (a scalar that is NaN or a NULL array: off).
static bool motion_on(const mac_motion* mo, bool* cone, bool* speed, bool* accel)
{
    *cone = *speed = *accel = false;
    if (!mo || !mo->anchor) return false;
    *cone = mo->cone_cos == mo->cone_cos && mo->vel;
    *speed = mo->v_max == mo->v_max;
    *accel = mo->a_max == mo->a_max && mo->speed_prev;
    return *cone || *speed || *accel;
}

// The kernels' arguments from a mac_motion with a constraint on: the per-UAV arrays built on the
// host (k_cons.h MotionArgs: anchor, vel, |vel|, cons6's thresholds) and uploaded into the lane's
// buffer on s. The host copies are read before the call returns.
static MotionArgs motion_upload(Lane* L, hipStream_t s, int N, const mac_motion* mo)
{
    bool cone, speed, accel;
    motion_on(mo, &cone, &speed, &accel);
    MotionArgs m{};
    m.cone = cone;
    m.speed = speed;
    m.accel = accel;
    m.cone_cos = mo->cone_cos;
    m.q5 = speed ? dlim_threshold(mo->v_max) : __builtin_inf();
    const size_t n = (size_t)N;
    std::vector<double>& h = L->h_motion;
    h.assign(8 * n, 0.0);
    std::copy(mo->anchor, mo->anchor + 3 * n, h.begin());
    if (cone) {
        std::copy(mo->vel, mo->vel + 2 * n, h.begin() + 3 * n);
        for (size_t i = 0; i < n; ++i) {
            const double ux = mo->vel[i], uy = mo->vel[n + i];
            h[5 * n + i] = std::sqrt(ux * ux + uy * uy);
        }
    }
    if (accel)
        for (size_t i = 0; i < n; ++i) motion_thresholds(mo->speed_prev[i], mo->a_max, &h[6 * n + i], &h[7 * n + i]);
    L->motion.reserve(sizeof(double) * 8 * std::max<size_t>(n, 1));
    HCK(hipMemcpyAsync(L->motion.p, h.data(), sizeof(double) * 8 * n, hipMemcpyHostToDevice, s));
    HCK(hipStreamSynchronize(s));   // (pageable source: the copy is done with h before anyone refills it)
    const double* d = L->motion.as<double>();
    m.anchor = d;
    m.vel = d + 3 * n;
    m.un = d + 5 * n;
    m.qhi = d + 6 * n;
    m.qlo = d + 7 * n;
    return m;
}

static void cons_mask_enqueue(hipStream_t s, const double* d_cands, int N, int64_t K, const ConsArgs& a,
                              uint8_t* d_feas, const MotionArgs* mot = nullptr)
{
    constexpr int64_t kMaxWG = (int64_t)1 << 23;   // workgroups per launch (2^31 threads)
    const int S = cons_slots(N);                   // UAVs per thread: 1, 2, 4, 8 (N <= 2048)
    const uint32_t lds = (mot && !a.sep) ? 0u : mask_lds(S);
    for (int64_t k0 = 0; k0 < K; k0 += kMaxWG) {
        const int64_t B = std::min(kMaxWG, K - k0);
        if (mot)
            hipLaunchKernelGGL(mask_motion_kern(S, a.sep), dim3((unsigned)B), dim3(kConsBlock), lds, s,
                               d_cands + (size_t)k0 * (size_t)(3 * N), N, a, *mot, d_feas + k0);
        else
            hipLaunchKernelGGL(mask_kern(S), dim3((unsigned)B), dim3(kConsBlock), lds, s,
                               d_cands + (size_t)k0 * (size_t)(3 * N), N, a, d_feas + k0);
        HCK(hipGetLastError());
    }
}

// obj[k] <- +inf at masked candidates, the argmin of the rest into best (and its mapped slot).
static void cons_argmin_enqueue(hipStream_t s, double* d_obj, const uint8_t* d_feas, int64_t K, int64_t idx_base,
                                void* d_best, uint64_t* d_mirror, uint64_t seq)
{
    hipLaunchKernelGGL(cons_argmin_kernel, dim3(1), dim3(kConsArgminBlock), 0, s, d_obj, d_feas, K, idx_base,
                       (unsigned long long*)d_best, d_mirror, seq);
    HCK(hipGetLastError());
}

// cons (masked poll, mac_poll_best_cons_f64; needs best_obj / best_idx): the mask launch before the
// chain, the masked argmin after it, in place on the lane's objectives and best.
template <class T>
static int32_t host_eval(mac_ctx* ctx, const T* cands, int64_t three_n, int64_t K,
                         const double* r_max, double penalty, const T* prev,
                         const double* d_lim, double tan_half_fov, double* area_out,
                         double* obj_out, double* best_obj, int64_t* best_idx,
                         const ConsArgs* cons = nullptr, const mac_motion* motion = nullptr)
{
    constexpr bool f32 = std::is_same<T, float>::value;
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (K == 0) {
        if (best_idx) *best_idx = -1;
        if (best_obj) *best_obj = INFINITY;
        return MAC_OK;
    }
    if (!cands) return fail(MAC_E_INVAL, "null candidates");
    const int N = (int)(three_n / 3);
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    L->cands.reserve(sizeof(double) * (size_t)std::max<int64_t>(three_n * K, 1));
    L->area.reserve(sizeof(double) * K);
    L->obj.reserve(sizeof(double) * K);
    L->best.reserve(16);
    // pinned staging (up to 64 MB): from pageable memory HIP would stage each copy
    // synchronously; one host memcpy into the lane's pinned buffer keeps the copies async
    const size_t in_bytes = sizeof(T) * (size_t)(three_n * K);
    const size_t out_bytes = sizeof(double) * (size_t)K * ((area_out ? 1 : 0) + (obj_out ? 1 : 0)) + 16;
    const bool staged = std::max(in_bytes, out_bytes) <= ((size_t)64 << 20);
    if (staged) L->h_io.reserve(std::max<size_t>(std::max(in_bytes, out_bytes), 64));
    const T* src_in = cands;
    if constexpr (!f32) {
        if (staged && in_bytes)
            staged_upload(cands, L->h_io.p, L->cands.p, in_bytes, s);
        else if (in_bytes)
            HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    } else {
        if (staged && in_bytes) {
            std::memcpy(L->h_io.p, cands, in_bytes);
            src_in = (const T*)L->h_io.p;
        }
        if (three_n * K > 0) upload_widen(src_in, three_n * K, L->c32, L->cands.as<double>(), s);
    }
    const bool want_obj = obj_out || best_obj || best_idx;
    double* d_rmax = nullptr;
    if (want_obj && r_max && N > 0) {
        L->rmax.reserve(sizeof(double) * N);
        HCK(hipMemcpyAsync(L->rmax.p, r_max, sizeof(double) * N, hipMemcpyHostToDevice, s));
        d_rmax = L->rmax.as<double>();
    }
    double* d_prev = nullptr;
    double* d_dlimT = nullptr;
    if (want_obj && prev && N > 0) {
        if (!d_lim) return fail(MAC_E_INVAL, "prev given without d_lim");
        cons3_upload(L, s, N, prev, d_lim);
        d_prev = L->prev.as<double>();
        d_dlimT = L->dlim.as<double>();
    }
    const double* hc = nullptr;
    if constexpr (!f32) hc = cands;   // (AUTO's host-side walk estimate reads fp64 candidates)
    if (K > 1 && !t_defer_free && !ctx->route_seeded.exchange(true)) {
        if constexpr (f32) {
            std::vector<double> x0(cands, cands + three_n);
            seed_route(ctx, x0.data(), N);
        } else {
            seed_route(ctx, cands, N);
        }
    }
    const bool tiled = use_tiled(ctx, N, hc, three_n);
    if (cons) {
        L->cmask.reserve((size_t)K);
        MotionArgs mot{};
        if (motion) mot = motion_upload(L, s, N, motion);   // (mac_poll_best_motion_f64: a constraint is on)
        cons_mask_enqueue(s, L->cands.as<double>(), N, K, *cons, L->cmask.as<uint8_t>(), motion ? &mot : nullptr);
    }
    EvalReq rq;
    rq.src = matrix_src(L->cands.as<double>(), N);
    rq.N = N;
    rq.K = (int)K;
    rq.tiled = tiled;
    rq.d_rmax = d_rmax;
    rq.penalty = penalty;
    rq.d_prev = d_prev;
    rq.d_dlimT = d_dlimT;
    rq.d_dlim_raw = d_prev ? L->dlimraw.as<double>() : nullptr;
    rq.tan_half_fov = tan_half_fov;
    rq.d_area = area_out ? L->area.as<double>() : nullptr;
    rq.d_obj = want_obj ? L->obj.as<double>() : nullptr;
    rq.d_best = (best_obj || best_idx) ? L->best.as<double>() : nullptr;
    enqueue_eval(ctx, L, s, rq);
    if (cons)
        cons_argmin_enqueue(s, L->obj.as<double>(), L->cmask.as<uint8_t>(), K, 0, L->best.p, nullptr, 0);
    // results: into the pinned buffer (the upload has completed before the kernels ran), then
    // one host copy each after the sync
    double* ho = staged ? (double*)L->h_io.p : nullptr;
    double* h_area = area_out ? (staged ? ho : area_out) : nullptr;
    double* h_obj = obj_out ? (staged ? ho + (area_out ? K : 0) : obj_out) : nullptr;
    double hb_local[2] = {0, 0};
    double* hb = staged ? ho + (size_t)K * ((area_out ? 1 : 0) + (obj_out ? 1 : 0)) : hb_local;
    if (h_area) HCK(hipMemcpyAsync(h_area, L->area.p, sizeof(double) * K, hipMemcpyDeviceToHost, s));
    if (h_obj) HCK(hipMemcpyAsync(h_obj, L->obj.p, sizeof(double) * K, hipMemcpyDeviceToHost, s));
    if (best_obj || best_idx) HCK(hipMemcpyAsync(hb, L->best.p, 16, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    if (staged && area_out) std::memcpy(area_out, h_area, sizeof(double) * K);
    if (staged && obj_out) std::memcpy(obj_out, h_obj, sizeof(double) * K);
    if (best_obj) *best_obj = hb[0];
    if (best_idx) *best_idx = __builtin_bit_cast(int64_t, hb[1]);
    return MAC_OK;
}


// The basis form of a caller-owned poll (mac_poll_basis_f64): the incumbent, B = L[rp][:, cp] as L's
// packed lower triangle (int16) with the two permutations, and delta; the 2n candidates
// x + delta B[:, k], x - delta B[:, k] are expanded on the device (k_prep.h CandSrc.entry), so the
// host ships n(n+1) + 16n bytes instead of the 3N x 2n matrix's 16 n^2.
static int32_t host_eval_basis(mac_ctx* ctx, const double* x_inc, int64_t three_n, const int16_t* ltri,
                               const int32_t* rp, const int32_t* cp, double delta, const double* r_max,
                               double penalty, const double* prev, const double* d_lim,
                               double tan_half_fov, double* obj_out, double* best_obj, int64_t* best_idx)
{
    const int64_t n = three_n;
    const int64_t K = 2 * n;
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (n == 0) {
        if (best_idx) *best_idx = -1;
        if (best_obj) *best_obj = INFINITY;
        return MAC_OK;
    }
    if (!x_inc || !ltri || !rp || !cp || !r_max) return fail(MAC_E_INVAL, "null argument");
    if (!std::isfinite(delta)) return fail(MAC_E_INVAL, "delta not finite");
    // the permutations index L on the device: every value must lie in [0, n)
    for (int64_t v = 0; v < n; ++v)
        if (rp[v] < 0 || rp[v] >= n || cp[v] < 0 || cp[v] >= n)
            return fail(MAC_E_INVAL, "rp / cp entry outside [0, n)");
    if (prev && !d_lim) return fail(MAC_E_INVAL, "prev given without d_lim");
    const int N = (int)(three_n / 3);
    int64_t bmax = 1;   // the largest |diagonal| (LTMADS: the step 2^ell): the chain's routing hint
    for (int64_t r = 0; r < n; ++r) bmax = std::max<int64_t>(bmax, std::abs((int)ltri[r * (r + 1) / 2 + r]));
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t tri = (size_t)n * (size_t)(n + 1) / 2;
    const size_t in_bytes = sizeof(double) * n + sizeof(int32_t) * 2 * n + sizeof(int16_t) * tri;
    const size_t out_bytes = (obj_out ? sizeof(double) * K : 0) + 16;
    L->cands.reserve(in_bytes);
    L->obj.reserve(sizeof(double) * K);
    L->best.reserve(16);
    // one pinned staging area and one copy: [x 8n][rp 4n][cp 4n][L 2 tri]
    L->h_io.reserve(std::max(in_bytes, out_bytes));
    unsigned char* h = (unsigned char*)L->h_io.p;
    std::memcpy(h, x_inc, sizeof(double) * n);
    std::memcpy(h + 8 * n, rp, sizeof(int32_t) * n);
    std::memcpy(h + 12 * n, cp, sizeof(int32_t) * n);
    std::memcpy(h + 16 * n, ltri, sizeof(int16_t) * tri);
    HCK(hipMemcpyAsync(L->cands.p, h, in_bytes, hipMemcpyHostToDevice, s));
    L->rmax.reserve(sizeof(double) * N);
    HCK(hipMemcpyAsync(L->rmax.p, r_max, sizeof(double) * N, hipMemcpyHostToDevice, s));
    double* d_prev = nullptr;
    double* d_dlimT = nullptr;
    if (prev) {
        cons3_upload(L, s, N, prev, d_lim);
        d_prev = L->prev.as<double>();
        d_dlimT = L->dlim.as<double>();
    }
    unsigned char* d = (unsigned char*)L->cands.p;
    EvalReq rq;
    CandSrc& src = rq.src;
    src.xinc = (const double*)d;
    src.rp = (const int*)(d + 8 * n);
    src.cp = (const int*)(d + 12 * n);
    src.ltri = (const int16_t*)(d + 16 * n);
    src.delta = delta;
    src.b = bmax;
    src.k0 = 0;
    src.route_five = host_crowded_disks(x_inc, N, (double)bmax * std::fabs(delta), ctx->grid.S) > kBitsMinDisks;
    rq.N = N;
    rq.K = (int)K;
    rq.tiled = use_tiled(ctx, N, nullptr, three_n);
    rq.d_rmax = L->rmax.as<double>();
    rq.penalty = penalty;
    rq.d_prev = d_prev;
    rq.d_dlimT = d_dlimT;
    rq.d_dlim_raw = d_prev ? L->dlimraw.as<double>() : nullptr;
    rq.tan_half_fov = tan_half_fov;
    rq.d_obj = L->obj.as<double>();
    rq.d_best = L->best.as<double>();
    enqueue_eval(ctx, L, s, rq);
    // (the upload completed before the kernels ran: the staging takes the results)
    double* ho = (double*)L->h_io.p;
    double* hb = ho + (obj_out ? K : 0);
    if (obj_out) HCK(hipMemcpyAsync(ho, L->obj.p, sizeof(double) * K, hipMemcpyDeviceToHost, s));
    HCK(hipMemcpyAsync(hb, L->best.p, 16, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    if (obj_out) std::memcpy(obj_out, ho, sizeof(double) * K);
    if (best_obj) *best_obj = hb[0];
    if (best_idx) *best_idx = __builtin_bit_cast(int64_t, hb[1]);
    return MAC_OK;
}

// ------------------------------------------------------------------ C-ABI

extern "C" {

#ifdef MAC_DIAG
// diagnostic build only (not declared in maxcover.h): per-workgroup poll-walk stamps
int32_t mac_diag_index_read(uint64_t* out, int64_t n)
{
    if (n > (int64_t)(8 * 65536)) n = 8 * 65536;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_index), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

int32_t mac_diag_walk_read(uint64_t* out, int64_t n)
{
    if (n > (int64_t)(8 * 65536)) n = 8 * 65536;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_walk), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: per-disk phase stamps of the fused kernel (k_fiw.h)
int32_t mac_diag_fiw_read(uint64_t* out, int64_t n)
{
    if (n > (int64_t)(16 * 65536)) n = 16 * 65536;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_fiw), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: per-block phase stamps of fin2_kernel (k_fiw.h)
int32_t mac_diag_f2_read(uint64_t* out, int64_t n)
{
    if (n > (int64_t)(8 * 4096)) n = 8 * 4096;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_f2), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: phase stamps of the prep launch's first 64 chain workgroups (k_prep.h)
int32_t mac_diag_prep_read(uint64_t* out, int64_t n)
{
    if (n > 64 * 16) n = 64 * 16;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_prep), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: per-workgroup phase ticks of shared_bits_kernel (k_bits.h)
int32_t mac_diag_bits_read(uint64_t* out, int64_t n)
{
    if (n > 256 * 16) n = 256 * 16;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_bits), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: per-workgroup phase ticks of shared_or_kernel (k_or.h)
int32_t mac_diag_or_read(uint64_t* out, int64_t n)
{
    if (n > 1024 * 16) n = 1024 * 16;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_or), sizeof(uint64_t) * n, 0,
                            hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

// diagnostic build only: the raw profiling stamps ({start, end} per workgroup slot, in launch
// order) and how many slots are used
int32_t mac_diag_stamps(mac_ctx* ctx, uint64_t* out, int64_t n, int64_t* used)
{
    if (!ctx) return MAC_E_INVAL;
    if (hipDeviceSynchronize() != hipSuccess) return MAC_E_HIP;
    std::lock_guard<std::mutex> lk(ctx->mu);
    *used = ctx->stamp_used;
    n = std::min<int64_t>(n, 2 * ctx->stamp_used);
    if (n > 0 && hipMemcpy(out, ctx->stamps.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}

int32_t mac_diag_read(uint64_t* out, int64_t n)
{
    if (n > (int64_t)(4 * kDiagMax)) n = 4 * kDiagMax;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), sizeof(uint64_t) * n, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return MAC_E_HIP;
    return MAC_OK;
}
#endif

// host only, every build (not declared in maxcover.h): the tile grid build_index chooses for a
// list of M entries with this bounding box of its finite entries; out = {S, invS, nTx, nTy}
int32_t mac_diag_grid(double xmn, double xmx, double ymn, double ymx, int64_t M, int32_t tile_points,
                      double* out)
{
    if (!out || tile_points < 1) return MAC_E_INVAL;
    const Grid g = choose_grid(xmn, xmx, ymn, ymx, M, tile_points);
    out[0] = g.S;
    out[1] = g.invS;
    out[2] = (double)g.nTx;
    out[3] = (double)g.nTy;
    return MAC_OK;
}

// host only, every build (not declared in maxcover.h): predicate.h's tile_of of the coordinate c and
// tile_span of the disk (c, r) along one axis of a grid; out = {tile_of, span found (0 / 1), lo, hi}
int32_t mac_diag_tiles(double c, double r, double g0, double invS, int32_t n, int32_t* out)
{
    if (!out || n < 1) return MAC_E_INVAL;
    int lo = -1, hi = -1;
    out[0] = tile_of(c, g0, invS, n);
    out[1] = tile_span(c, r, g0, invS, n, lo, hi) ? 1 : 0;
    out[2] = lo;
    out[3] = hi;
    return MAC_OK;
}

// host only, every build (not declared in maxcover.h): the route enqueue_eval plans (eval_plan.h)
// for in = {algo, chain, cus, M, w_uniform, kind (RouteIn::Kind), np, k0, mesh, mst, route_five, b,
// want_area, want_obj, cons3, mask, tiled, N, K} and the basis form's delta; the first n_out of
// out = {poll_possible, walk_forced, iper, want_keys, pair, gen_x, mesh, nchain, G, units,
// fused_eligible, excl, counts, prep_fused (PrepKind), nprep, xbase, prep_five_runs, prep_five, nrec,
// nfw, nidx, nfin2, nfin}
static RouteIn diag_route_in(const int64_t* in, double delta)
{
    RouteIn ri;
    ri.algo = (int)in[0];
    ri.chain = (int)in[1];
    ri.cus = (int)in[2];
    ri.M = in[3];
    ri.w_uniform = in[4] != 0;
    ri.kind = (int)in[5];
    ri.np = (int)in[6];
    ri.k0 = (int)in[7];
    ri.mesh = in[8] != 0;
    ri.mst = in[9] != 0;
    ri.route_five = in[10] != 0;
    ri.b = in[11];
    ri.delta = delta;
    ri.want_area = in[12] != 0;
    ri.want_obj = in[13] != 0;
    ri.cons3 = in[14] != 0;
    ri.mask = in[15] != 0;
    ri.tiled = in[16] != 0;
    ri.N = (int)in[17];
    ri.K = (int)in[18];
    return ri;
}

static int32_t diag_route_out(const RouteIn& ri, int64_t* out, int32_t n_out)
{
    const EvalPlan p = eval_plan(ri);
    const int64_t v[] = {p.poll_possible, p.walk_forced, p.iper, p.want_keys, p.pair, p.gen_x, p.mesh, p.nchain,
                         p.G, p.units, p.fused_eligible, p.excl, p.counts, p.prep_fused, p.nprep, p.xbase,
                         p.prep_five_runs, p.prep_five, p.nrec, p.nfw, p.nidx, p.nfin2, p.nfin};
    for (int q = 0; q < n_out && q < (int)(sizeof v / sizeof v[0]); ++q) out[q] = v[q];
    return MAC_OK;
}

int32_t mac_diag_route(const int64_t* in, double delta, int64_t* out, int32_t n_out)
{
    if (!in || !out || n_out < 0 || in[17] < 0 || in[18] < 1) return MAC_E_INVAL;
    return diag_route_out(diag_route_in(in, delta), out, n_out);
}

// The chain word of a run on the mesh g (its n_p polled entries; null: none) whose layout the host found
// crowded or not: a non-integer granularity sends value keys to the five-launch chain (mac_mads_begin*);
// mesh keys (MAC_OPT_MESH_KEYS) pack at every granularity and follow the crowding estimate alone.
static int mads_route_five(bool crowded, const double* g, int np, bool mesh_keys)
{
    int five = crowded ? 1 : 0;
    for (int v = 0; v < np && g && !mesh_keys; ++v)
        if (g[v] != std::floor(g[v])) five = 1;
    return five;
}

// host only, every build (not declared in maxcover.h): mac_diag_route with the key mode. `in` as above
// (its route_five word is ignored) with in[19] = MAC_OPT_MESH_KEYS's value appended; g: the n_g polled
// granularities of a run's mesh (n_g = 0: no mesh) and `crowded` its begin's crowding verdict, from which
// the run's chain word follows as in mac_mads_begin* (mads_route_five; returned in *route_five). out's
// mesh word is the kMesh argument of the chains' builds: 0 none, 1 value keys, 2 mesh keys.
int32_t mac_diag_route_keys(const int64_t* in, double delta, int64_t* out, int32_t n_out, const double* g,
                            int32_t n_g, int32_t crowded, int32_t* route_five)
{
    if (!in || !out || n_out < 0 || in[17] < 0 || in[18] < 1 || n_g < 0 || (n_g && !g)) return MAC_E_INVAL;
    if (in[19] != MAC_KEYS_VALUE && in[19] != MAC_KEYS_MESH) return MAC_E_INVAL;
    RouteIn ri = diag_route_in(in, delta);
    ri.mesh = n_g > 0;
    ri.mesh_keys = in[19] == MAC_KEYS_MESH && n_g > 0;
    ri.route_five = mads_route_five(crowded != 0, n_g ? g : nullptr, n_g, ri.mesh_keys) != 0;
    if (route_five) *route_five = ri.route_five ? 1 : 0;
    return diag_route_out(ri, out, n_out);
}

// host only, every build (not declared in maxcover.h): mesh_key.h as the kernels inline it, over n
// triples: x, g, v = [n][3] doubles (the incumbent's disk, its granularities, the candidate's doubles;
// v null: the decode itself), m = [n][3] signed draws. word[n]: the packed word, or the escape when a
// draw is past its field or a decode is not v bit for bit; dec[n][3]: the decodes; flags[n]: bit 0 the
// draws pack, bit 1 every decode reproduces v.
int32_t mac_diag_mesh_key(int64_t n, const double* x, const double* g, const int32_t* m, const double* v,
                          uint32_t* word, double* dec, int32_t* flags)
{
    if (n < 0 || !x || !g || !m || !word || !dec || !flags) return MAC_E_INVAL;
    for (int64_t t = 0; t < n; ++t) {
        // (the kernels build a word a field at a time, mesh_key_put: the draw's range and the decode's
        // bits in one; mesh_key_pack is the same word from the three integers)
        uint32_t w = 0u, wp = 0u;
        bool put = true, exact = true;
        for (int q = 0; q < 3; ++q) {
            const int64_t at = 3 * t + q;
            dec[at] = mesh_key_decode(x[at], g[at], (double)m[at]);
            const double want = v ? v[at] : dec[at];
            exact = mesh_key_exact(x[at], g[at], m[at], want) && exact;
            put = mesh_key_put(w, q, x[at], g[at], (double)m[at], want) && put;
        }
        const bool packed = mesh_key_pack(m[3 * t], m[3 * t + 1], m[3 * t + 2], wp);
        if (put != (packed && exact) || (put && w != wp)) return MAC_E_INVAL;   // (never: one encoding)
        word[t] = put ? w : kMeshKeyEsc;
        flags[t] = (packed ? 1 : 0) | (exact ? 2 : 0);
    }
    return MAC_OK;
}

// host only, every build (not declared in maxcover.h): the workgroups that took stamps under each
// launch role (mac_profile_kernels' roles) in the launches recorded since the last reset, summed
int32_t mac_diag_role_slots(mac_ctx* ctx, int64_t* out, int32_t n_roles)
{
    if (!ctx || !out || n_roles < 0) return MAC_E_INVAL;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int r = 0; r < n_roles; ++r) out[r] = 0;
    for (auto& p : ctx->prof)
        for (int r = 0; r < n_roles && r < MAC_PROF_ROLES; ++r)
            if (p.role[r][0] >= 0) out[r] += p.role[r][1];
    return MAC_OK;
}

// host only (declared in maxcover.h): what the context's most recent five-launch poll left on its
// lane, copied back after a device synchronisation: words[0] the walk (k_common.h kMode*),
// words[1 ..] the poll walk's counters (kDc*), and the index's positions per disk. Launches
// nothing and changes nothing a poll reads.
int32_t mac_diag_poll_report(mac_ctx* ctx, int32_t* words, int32_t n_words, int32_t* ucount, int32_t n_disks)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (n_words < 0 || n_disks < 0 || (n_words > 0 && !words) || (n_disks > 0 && !ucount))
        return fail(MAC_E_INVAL, "mac_diag_poll_report: a count without its array");
    set_device(ctx);
    HCK(hipDeviceSynchronize());
    const Lane* L = ctx->last_five.load(std::memory_order_relaxed);
    if (!L) return fail(MAC_E_INVAL, "mac_diag_poll_report: no five-launch poll has run on this context");
    if (sizeof(int) * (size_t)n_disks > L->ucount.cap)
        return fail(MAC_E_INVAL, "mac_diag_poll_report: more disks than the poll had");
    const int nw = std::min<int>(n_words, 1 + kDcCount);
    for (int q = nw; q < n_words; ++q) words[q] = 0;
    if (nw > 0) HCK(hipMemcpy(words, L->mode.p, sizeof(int) * (size_t)nw, hipMemcpyDeviceToHost));
    if (n_disks > 0) HCK(hipMemcpy(ucount, L->ucount.p, sizeof(int) * (size_t)n_disks, hipMemcpyDeviceToHost));
    return MAC_OK;
    ABI_END
}

const char* mac_last_error(void) { return g_last_error.c_str(); }

const char* mac_version(void) { return "maxcover 0.1.0 gfx950"; }

double mac_cover_threshold(double r) { return cover_threshold(r); }

int32_t mac_profile_read(mac_ctx* ctx, double* kernel_ms, int64_t* launches,
                         int64_t* candidates, int32_t* last_algo, int32_t reset)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    set_device(ctx);
    HCK(hipDeviceSynchronize());   // every recorded launch has completed
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<uint64_t> st((size_t)(2 * ctx->stamp_used));
    if (!st.empty())
        HCK(hipMemcpy(st.data(), ctx->stamps.p, sizeof(uint64_t) * st.size(), hipMemcpyDeviceToHost));
    double ms = 0.0;
    int64_t n = 0, kc = 0;
    int algo = 0;
    // launch time = last wave end - first workgroup start over the launch's workgroups
    auto span_ms = [&](int64_t base, int64_t nwg) {
        uint64_t t0 = ~(uint64_t)0, t1 = 0;
        for (int64_t q = base; q < base + nwg; ++q) {
            t0 = std::min(t0, st[(size_t)(2 * q)]);
            t1 = std::max(t1, st[(size_t)(2 * q + 1)]);
        }
        return t1 > t0 ? (double)(t1 - t0) / kRealtimeHz * 1e3 : 0.0;
    };
    for (auto& p : ctx->prof) {
        algo = p.algo;
        int64_t a = p.a, na = p.na;
        if (p.mode) {  // the device's choice (the lane's mode word holds its latest decision)
            int m = 0;
            HCK(hipMemcpy(&m, p.mode, sizeof(int), hipMemcpyDeviceToHost));
            algo = m == kModePoll ? MAC_ALGO_POLL : MAC_ALGO_TILED;
            if (m == kModePoll) {
                a = p.b;
                na = p.nb;
            }
        }
        if (a < 0) continue;
        ms += span_ms(a, na);
        ++n;
        kc += p.K;
    }
    if (kernel_ms) *kernel_ms = ms;
    if (launches) *launches = n;
    if (candidates) *candidates = kc;
    if (last_algo) *last_algo = algo;
    if (reset) {
        ctx->prof.clear();
        if (ctx->stamp_used) HCK(hipMemset(ctx->stamps.p, 0, sizeof(uint64_t) * 2 * ctx->stamp_used));
        ctx->stamp_used = 0;
    }
    return MAC_OK;
    ABI_END
}

int32_t mac_profile_split(mac_ctx* ctx, double* prep_ms, double* walk_ms, double* gap_ms,
                          int64_t* polls)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    set_device(ctx);
    HCK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<uint64_t> st((size_t)(2 * ctx->stamp_used));
    if (!st.empty())
        HCK(hipMemcpy(st.data(), ctx->stamps.p, sizeof(uint64_t) * st.size(), hipMemcpyDeviceToHost));
    double a1 = 0.0, a2 = 0.0, gap = 0.0;
    int64_t n = 0;
    for (auto& p : ctx->prof) {
        // the launch chain: prep = first launch's start .. the walk's start, walk = the walk
        // launch, gap = the walk's end .. finalize's end (the argmin included)
        if (p.c < 0 || p.f < 0) continue;
        int64_t wa = p.a, wn = p.na;
        if (p.mode) {
            int m = 0;
            HCK(hipMemcpy(&m, p.mode, sizeof(int), hipMemcpyDeviceToHost));
            if (m == kModePoll) {
                wa = p.b;
                wn = p.nb;
            }
        }
        uint64_t s0 = ~(uint64_t)0, sw = ~(uint64_t)0, ew = 0, ef = 0;
        for (int64_t q = p.c; q < p.c + p.nc; ++q) s0 = std::min(s0, st[(size_t)(2 * q)]);
        for (int64_t q = wa; wa >= 0 && q < wa + wn; ++q) {
            sw = std::min(sw, st[(size_t)(2 * q)]);
            ew = std::max(ew, st[(size_t)(2 * q + 1)]);
        }
        for (int64_t q = p.f; q < p.f + p.nf; ++q) ef = std::max(ef, st[(size_t)(2 * q + 1)]);
        if (!(ef > s0) || !(ew > sw) || sw < s0) continue;
        a1 += (double)(sw - s0) / kRealtimeHz * 1e3;
        a2 += (double)(ew - sw) / kRealtimeHz * 1e3;
        gap += (double)(ef - ew) / kRealtimeHz * 1e3;
        ++n;
    }
    if (prep_ms) *prep_ms = a1;
    if (walk_ms) *walk_ms = a2;
    if (gap_ms) *gap_ms = gap;
    if (polls) *polls = n;
    return MAC_OK;
    ABI_END
}

int32_t mac_profile_fused(mac_ctx* ctx, int64_t* reports, int64_t* ident_sum, int64_t* ident_max, int32_t reset)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (reports) *reports = ctx->fw_reports.load(std::memory_order_relaxed);
    if (ident_sum) *ident_sum = ctx->fw_ident_sum.load(std::memory_order_relaxed);
    if (ident_max) *ident_max = ctx->fw_ident_max.load(std::memory_order_relaxed);
    if (reset) {
        ctx->fw_reports.store(0, std::memory_order_relaxed);
        ctx->fw_ident_sum.store(0, std::memory_order_relaxed);
        ctx->fw_ident_max.store(0, std::memory_order_relaxed);
    }
    return MAC_OK;
}

int32_t mac_profile_kernels(mac_ctx* ctx, double* ms_out, int64_t* launches_out, int32_t n_roles)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (n_roles < 0 || (n_roles > 0 && (!ms_out || !launches_out)))
        return fail(MAC_E_INVAL, "null output / negative role count");
    set_device(ctx);
    HCK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<uint64_t> st((size_t)(2 * ctx->stamp_used));
    if (!st.empty())
        HCK(hipMemcpy(st.data(), ctx->stamps.p, sizeof(uint64_t) * st.size(), hipMemcpyDeviceToHost));
    const int nr = std::min<int32_t>(n_roles, MAC_PROF_ROLES);
    for (int r = 0; r < n_roles; ++r) {
        ms_out[r] = 0.0;
        launches_out[r] = 0;
    }
    for (auto& p : ctx->prof) {
        for (int r = 0; r < nr; ++r) {
            const int64_t base = p.role[r][0], nwg = p.role[r][1];
            if (base < 0 || nwg <= 0) continue;
            uint64_t t0 = ~(uint64_t)0, t1 = 0;
            for (int64_t q = base; q < base + nwg; ++q) {
                t0 = std::min(t0, st[(size_t)(2 * q)]);
                t1 = std::max(t1, st[(size_t)(2 * q + 1)]);
            }
            if (!(t1 > t0)) continue;
            ms_out[r] += (double)(t1 - t0) / kRealtimeHz * 1e3;
            ++launches_out[r];
        }
    }
    return MAC_OK;
    ABI_END
}

int32_t mac_device_count(int32_t* count_out)
{
    ABI_BEGIN
    if (!count_out) return fail(MAC_E_INVAL, "null count_out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count_out = n;
    return MAC_OK;
    ABI_END
}

int32_t mac_ctx_create(mac_ctx** out, int32_t device)
{
    ABI_BEGIN
    if (!out) return fail(MAC_E_INVAL, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MAC_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(MAC_E_NODEVICE, "device index out of range");
    HCK(hipSetDevice(device));
    mac_ctx* ctx = new mac_ctx();
    if (const char* e = std::getenv("MAXCOVER_HOST_STATS"); e && *e == '1') ctx->host_stats = true;
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->cus = prop.multiProcessorCount;
    int bar = 0;
    const char* eb = std::getenv("MAXCOVER_CL_BAR");
    ctx->cl_bar = hipDeviceGetAttribute(&bar, hipDeviceAttributeIsLargeBar, device) == hipSuccess && bar == 1 &&
                  !(eb && *eb == '0');
    HCK(hipStreamCreateWithFlags(&ctx->setup_stream, hipStreamNonBlocking));
    *out = ctx;
    return MAC_OK;
    ABI_END
}

void mac_ctx_destroy(mac_ctx* ctx)
{
    if (!ctx) return;
    if (const char* e = std::getenv("MAXCOVER_CL_STATS"); e && *e == '1' && ctx->cl_batches) {
        std::fprintf(stderr, "maxcover: closure batches %lld, requests %lld (%.2f per batch); per batch (us): "
                     "lane %.1f, staging %.1f, copy+launch %.1f, hand-out %.1f\n",
                     (long long)ctx->cl_batches, (long long)ctx->cl_reqs, (double)ctx->cl_reqs / (double)ctx->cl_batches,
                     ctx->cl_phase_ns[3] * 1e-3 / ctx->cl_batches, ctx->cl_phase_ns[0] * 1e-3 / ctx->cl_batches,
                     ctx->cl_phase_ns[1] * 1e-3 / ctx->cl_batches, ctx->cl_phase_ns[2] * 1e-3 / ctx->cl_batches);
        const double u = 1e-3 / (double)ctx->cl_reqs;
        std::fprintf(stderr, "maxcover: closure per request (us): queued %.1f, taken -> handed out %.1f, "
                     "-> seen %.1f, -> slot read %.1f; call %.1f; led by own thread %.0f%%\n",
                     ctx->cl_req_ns[0] * u, ctx->cl_req_ns[1] * u, ctx->cl_req_ns[2] * u, ctx->cl_req_ns[3] * u,
                     ctx->cl_req_ns[4] * u, 100.0 * ctx->cl_led / ctx->cl_reqs);
    }
    if (ctx->host_stats && ctx->hs_n)
        std::fprintf(stderr, "maxcover: fused polls %lld, host us per poll: to prep launch %.2f, prep launch %.2f, "
                     "fiw launch %.2f, fin2 launch %.2f\n", (long long)ctx->hs_n, ctx->hs_t[0] / ctx->hs_n * 1e6,
                     ctx->hs_t[1] / ctx->hs_n * 1e6, ctx->hs_t[2] / ctx->hs_n * 1e6, ctx->hs_t[3] / ctx->hs_n * 1e6);
    (void)hipSetDevice(ctx->device);
    if (ctx->doorbell) {   // every armed poll released first (else the synchronisation would wait)
        __atomic_store_n(ctx->doorbell, ~(uint64_t)0 >> 1, __ATOMIC_RELEASE);
        ctx->fired = ctx->armed;
    }
    (void)hipDeviceSynchronize();
    if (ctx->comm) (void)ctx->rccl->comm_destroy(ctx->comm);
    if (ctx->d_xrec) (void)hipFree(ctx->d_xrec);
    if (ctx->d_xrec2) (void)hipFree(ctx->d_xrec2);
    ctx->h_xrec.release();
    free_deferred(ctx);
    if (ctx->doorbell) (void)hipHostFree(ctx->doorbell);
    ctx->h_mirror.release();
    for (Lane* l : ctx->lanes_all) {
        l->h_stage.release();
        l->h_io.release();
        l->h_dc.release();
        l->h_cl.release();
        for (DevBuf* b : {&l->cands, &l->disks, &l->partial, &l->area, &l->obj, &l->best,
                          &l->rmax, &l->prev, &l->dlim, &l->region, &l->mode, &l->nbr,
                          &l->ncount, &l->dlist, &l->qual, &l->spart, &l->vp, &l->xinc,
                          &l->perm, &l->ucount, &l->umap, &l->keysT, &l->lane4,
                          &l->lanexp, &l->rows, &l->nboxT, &l->cnt, &l->dlimraw, &l->finblk, &l->finarrive, &l->c32, &l->p32,
                          &l->cpart, &l->carrive, &l->ctot, &l->clv, &l->prec, &l->cost, &l->nboxU,
                          &l->ncountU, &l->orjobs, &l->pd, &l->dead8, &l->frows, &l->fwhint, &l->fwlist, &l->fwcount,
                          &l->fwsxy, &l->fwsw, &l->bdpart, &l->bdarrive, &l->bdout, &l->cmask, &l->cbest,
                          &l->motion, &l->verdict, &l->prog, &l->progh, &l->progobj, &l->progrec})
            b->release();
        if (l->done) (void)hipEventDestroy(l->done);

        if (l->stream) (void)hipStreamDestroy(l->stream);
        delete l;
    }
    for (DevBuf* b : {&ctx->x, &ctx->y, &ctx->w, &ctx->xys, &ctx->ws, &ctx->perm, &ctx->off,
                      &ctx->keys_in, &ctx->keys_out, &ctx->idx_in, &ctx->tmp, &ctx->bbox,
                      &ctx->flags_s, &ctx->flags_o, &ctx->keep, &ctx->sel_count, &ctx->cx,
                      &ctx->cy, &ctx->cw, &ctx->cidx, &ctx->circ, &ctx->cdisk, &ctx->rboxes,
                      &ctx->rcount, &ctx->ritems, &ctx->rpart, &ctx->rout, &ctx->vtally})
        b->release();
    ctx->stamps.release();
    if (ctx->setup_stream) (void)hipStreamDestroy(ctx->setup_stream);
    delete ctx;
}

int32_t mac_set_option(mac_ctx* ctx, int32_t option, int64_t value)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    switch (option) {
    case MAC_OPT_ALGO:
        if (value < MAC_ALGO_AUTO || value > MAC_ALGO_POLL) return fail(MAC_E_INVAL, "bad algo");
        ctx->algo = (int)value;
        return MAC_OK;
    case MAC_OPT_STORAGE:
        if (value != MAC_STORE_F64 && value != MAC_STORE_F32)
            return fail(MAC_E_INVAL, "bad storage");
        // the list stays fp64 in HBM: the walks' band decisions re-read exact coordinates, and
        // fp32 inputs arrive through the *_f32 entry points, widened losslessly
        if (value == MAC_STORE_F32) return fail(MAC_E_INVAL, "storage is fp64 (use the *_f32 entry points)");
        ctx->storage = (int)value;
        return MAC_OK;
    case MAC_OPT_PROFILE: {
        ABI_BEGIN
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (value && !ctx->profile) {  // fresh, zeroed stamp slots (outside any timed region)
            set_device(ctx);
            constexpr int64_t kSlots = (int64_t)1 << 21;   // 32 MB: ~800 config-4 poll chains
            ctx->stamps.reserve(sizeof(uint64_t) * 2 * kSlots);
            HCK(hipDeviceSynchronize());
            HCK(hipMemset(ctx->stamps.p, 0, sizeof(uint64_t) * 2 * kSlots));
            ctx->stamp_cap = kSlots;
            ctx->stamp_used = 0;
            ctx->prof.clear();
        }
        ctx->profile = value != 0;
        return MAC_OK;
        ABI_END
    }
    case MAC_OPT_SHARED:
        if (value < MAC_SHARED_AUTO || value > MAC_SHARED_BITS) return fail(MAC_E_INVAL, "bad shared mode");
        ctx->shared_mode = (int)value;
        return MAC_OK;
    case MAC_OPT_CHAIN:
        if (value < MAC_CHAIN_AUTO || value > MAC_CHAIN_FUSED) return fail(MAC_E_INVAL, "bad chain");
        ctx->chain = (int)value;
        return MAC_OK;
    case MAC_OPT_MESH_KEYS:
        if (value != MAC_KEYS_VALUE && value != MAC_KEYS_MESH) return fail(MAC_E_INVAL, "bad mesh keys mode");
        ctx->mesh_keys = (int)value;
        return MAC_OK;
    case MAC_OPT_VERDICTS:
        if (value != 0 && value != 1) return fail(MAC_E_INVAL, "bad verdicts mode");
        ctx->verdicts.store((int)value, std::memory_order_relaxed);
        return MAC_OK;
    case MAC_OPT_TILE_POINTS:
        if (value < 1 || value > 4096) return fail(MAC_E_INVAL, "tile points out of range");
        ctx->tile_ppt = (int)value;
        return MAC_OK;
    default:
        return fail(MAC_E_INVAL, "unknown option");
    }
}

// High-interest regions on (mac_set_regions): the entries [lo, hi) that just arrived in the list-order
// arrays are tested once, before the index is built (w_uniform and the sorted weights see the final
// weights): inside any box they take the high-interest weight and are counted. reset: a new list
// (the counters restart at its counts); an append adds.
static void regions_ingest(mac_ctx* ctx, hipStream_t s, int64_t lo, int64_t hi, bool reset)
{
    if (ctx->n_regions == 0) return;
    if (reset) HCK(hipMemsetAsync(ctx->rcount.p, 0, sizeof(unsigned long long) * (kRegionsMax + 1), s));
    if (hi <= lo) return;
    const unsigned nb = std::min<unsigned>(grid1d(hi - lo, kBlock), kRegIngestBlocks);
    hipLaunchKernelGGL(region_ingest_kernel, dim3(nb), dim3(kBlock), 0, s, ctx->x.as<double>(),
                       ctx->y.as<double>(), ctx->w.as<double>(), lo, hi, ctx->rboxes.as<double>(),
                       ctx->n_regions, ctx->reg_w_high, std::isnan(ctx->reg_w_high) ? 0 : 1,
                       ctx->rcount.as<unsigned long long>());
    HCK(hipGetLastError());
}

static int32_t set_points_common(mac_ctx* ctx, int64_t M)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    int32_t rc = check_M(M);
    if (rc) return rc;
    set_device(ctx);
    HCK(hipDeviceSynchronize());  // no evaluation may overlap a point-list change
    free_deferred(ctx);
    ctx->M = M;
    ctx->has_points = false;
    const size_t b = sizeof(double) * (size_t)std::max<int64_t>(M, 1);
    ctx->x.reserve(b);
    ctx->y.reserve(b);
    ctx->w.reserve(b);
    return MAC_OK;
}

int32_t mac_set_points_f64(mac_ctx* ctx, const double* x, const double* y, const double* w,
                           int64_t M)
{
    ABI_BEGIN
    if (M > 0 && (!x || !y || !w)) return fail(MAC_E_INVAL, "null point array");
    int32_t rc = set_points_common(ctx, M);
    if (rc) return rc;
    hipStream_t s = ctx->setup_stream;
    if (M > 0) {
        HCK(hipMemcpyAsync(ctx->x.p, x, sizeof(double) * M, hipMemcpyHostToDevice, s));
        HCK(hipMemcpyAsync(ctx->y.p, y, sizeof(double) * M, hipMemcpyHostToDevice, s));
        HCK(hipMemcpyAsync(ctx->w.p, w, sizeof(double) * M, hipMemcpyHostToDevice, s));
    }
    regions_ingest(ctx, s, 0, M, true);
    build_index(ctx, s);
    return MAC_OK;
    ABI_END
}

int32_t mac_set_points_f32(mac_ctx* ctx, const float* x, const float* y, const float* w, int64_t M)
{
    ABI_BEGIN
    if (M > 0 && (!x || !y || !w)) return fail(MAC_E_INVAL, "null point array");
    int32_t rc = set_points_common(ctx, M);
    if (rc) return rc;
    hipStream_t s = ctx->setup_stream;
    upload_widen(x, M, ctx->tmp, ctx->x.as<double>(), s);
    HCK(hipStreamSynchronize(s));   // (one staging buffer, reused per coordinate)
    upload_widen(y, M, ctx->tmp, ctx->y.as<double>(), s);
    HCK(hipStreamSynchronize(s));
    upload_widen(w, M, ctx->tmp, ctx->w.as<double>(), s);
    regions_ingest(ctx, s, 0, M, true);
    build_index(ctx, s);
    return MAC_OK;
    ABI_END
}

int32_t mac_set_points_dev_f32(mac_ctx* ctx, const float* d_x, const float* d_y, const float* d_w,
                               int64_t M)
{
    ABI_BEGIN
    if (M > 0 && (!d_x || !d_y || !d_w)) return fail(MAC_E_INVAL, "null point array");
    int32_t rc = set_points_common(ctx, M);
    if (rc) return rc;
    hipStream_t s = ctx->setup_stream;
    widen_async(d_x, M, ctx->x.as<double>(), s);
    widen_async(d_y, M, ctx->y.as<double>(), s);
    widen_async(d_w, M, ctx->w.as<double>(), s);
    regions_ingest(ctx, s, 0, M, true);
    build_index(ctx, s);
    return MAC_OK;
    ABI_END
}

int32_t mac_set_points_records_f64(mac_ctx* ctx, const double* rec, int64_t M, int64_t stride)
{
    ABI_BEGIN
    if (M > 0 && !rec) return fail(MAC_E_INVAL, "null records");
    if (stride < 4) return fail(MAC_E_INVAL, "record stride < 4");
    std::vector<double> hx(std::max<int64_t>(M, 0)), hy(hx.size()), hw(hx.size());
    for (int64_t i = 0; i < M; ++i) {
        hx[i] = rec[i * stride + 0];
        hy[i] = rec[i * stride + 1];
        hw[i] = rec[i * stride + 3];  // column 4, src/AreaCoverageCalculation.jl:72
    }
    return mac_set_points_f64(ctx, hx.data(), hy.data(), hw.data(), M);
    ABI_END
}

int32_t mac_set_points_dev_f64(mac_ctx* ctx, const double* d_x, const double* d_y,
                               const double* d_w, int64_t M)
{
    ABI_BEGIN
    if (M > 0 && (!d_x || !d_y || !d_w)) return fail(MAC_E_INVAL, "null point array");
    int32_t rc = set_points_common(ctx, M);
    if (rc) return rc;
    hipStream_t s = ctx->setup_stream;
    if (M > 0) {
        HCK(hipMemcpyAsync(ctx->x.p, d_x, sizeof(double) * M, hipMemcpyDeviceToDevice, s));
        HCK(hipMemcpyAsync(ctx->y.p, d_y, sizeof(double) * M, hipMemcpyDeviceToDevice, s));
        HCK(hipMemcpyAsync(ctx->w.p, d_w, sizeof(double) * M, hipMemcpyDeviceToDevice, s));
    }
    regions_ingest(ctx, s, 0, M, true);
    build_index(ctx, s);
    return MAC_OK;
    ABI_END
}

// update_POI (src/CellFunctions.jl:59-79): the list grows at its end; the existing entries keep
// their positions (list order = summation order), then the tile index is rebuilt.
static int32_t append_common(mac_ctx* ctx, const void* x, const void* y, const void* w, int64_t m,
                             hipMemcpyKind kind)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (m < 0) return fail(MAC_E_INVAL, "m < 0");
    if (m > 0 && (!x || !y || !w)) return fail(MAC_E_INVAL, "null point array");
    const int64_t M0 = ctx->has_points ? ctx->M : 0;
    int32_t rc = check_M(M0 + m);
    if (rc) return rc;
    set_device(ctx);
    HCK(hipDeviceSynchronize());  // no evaluation may overlap a point-list change
    free_deferred(ctx);
    hipStream_t s = ctx->setup_stream;
    const size_t need = sizeof(double) * (size_t)std::max<int64_t>(M0 + m, 1);
    if (need > ctx->x.cap) {      // grow by 1.5x, keeping the existing entries
        const size_t b = std::max(need, ctx->x.cap + ctx->x.cap / 2);
        for (DevBuf* d : {&ctx->x, &ctx->y, &ctx->w}) {
            DevBuf nb;
            nb.reserve(b);
            if (M0 > 0) HCK(hipMemcpyAsync(nb.p, d->p, sizeof(double) * M0, hipMemcpyDeviceToDevice, s));
            HCK(hipStreamSynchronize(s));
            d->release();
            *d = nb;
            nb.p = nullptr;
            nb.cap = 0;
        }
    }
    if (m > 0) {
        HCK(hipMemcpyAsync(ctx->x.as<double>() + M0, x, sizeof(double) * m, kind, s));
        HCK(hipMemcpyAsync(ctx->y.as<double>() + M0, y, sizeof(double) * m, kind, s));
        HCK(hipMemcpyAsync(ctx->w.as<double>() + M0, w, sizeof(double) * m, kind, s));
    }
    ctx->M = M0 + m;
    regions_ingest(ctx, s, M0, M0 + m, false);
    build_index(ctx, s);
    return MAC_OK;
}

int32_t mac_append_points_f64(mac_ctx* ctx, const double* x, const double* y, const double* w,
                              int64_t m)
{
    ABI_BEGIN
    return append_common(ctx, x, y, w, m, hipMemcpyHostToDevice);
    ABI_END
}

int32_t mac_append_points_dev_f64(mac_ctx* ctx, const double* d_x, const double* d_y,
                                  const double* d_w, int64_t m)
{
    ABI_BEGIN
    return append_common(ctx, d_x, d_y, d_w, m, hipMemcpyDeviceToDevice);
    ABI_END
}

int32_t mac_num_points(mac_ctx* ctx, int64_t* M_out)
{
    if (!ctx || !M_out) return fail(MAC_E_INVAL, "null argument");
    *M_out = ctx->has_points ? ctx->M : 0;
    return MAC_OK;
}

int32_t mac_get_points_f64(mac_ctx* ctx, double* x, double* y, double* w)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (!ctx->has_points) return fail(MAC_E_NOPOINTS, "no point list set");
    set_device(ctx);
    hipStream_t s = ctx->setup_stream;
    const size_t b = sizeof(double) * ctx->M;
    if (ctx->M > 0) {
        if (x) HCK(hipMemcpyAsync(x, ctx->x.p, b, hipMemcpyDeviceToHost, s));
        if (y) HCK(hipMemcpyAsync(y, ctx->y.p, b, hipMemcpyDeviceToHost, s));
        if (w) HCK(hipMemcpyAsync(w, ctx->w.p, b, hipMemcpyDeviceToHost, s));
    }
    HCK(hipStreamSynchronize(s));
    return MAC_OK;
    ABI_END
}

// covered flags (list order) into ctx->flags_o for one candidate; returns on stream s.
static void compute_flags(mac_ctx* ctx, hipStream_t s, const double* circles, int N)
{
    const int64_t M = ctx->M;
    ctx->flags_s.reserve(std::max<int64_t>(M, 1));
    ctx->flags_o.reserve(std::max<int64_t>(M, 1));
    ctx->circ.reserve(sizeof(double) * std::max(3 * N, 1));
    ctx->cdisk.reserve(sizeof(DiskRec) * std::max(N, 1));
    if (M == 0) return;
    HCK(hipMemsetAsync(ctx->flags_s.p, 0, M, s));
    if (N > 0) {
        HCK(hipMemcpyAsync(ctx->circ.p, circles, sizeof(double) * 3 * N, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(disk_prep_kernel, dim3(grid1d(N, 256)), dim3(256), 0, s,
                           matrix_src(ctx->circ.as<double>(), N), N, 1, ctx->cdisk.as<DiskRec>());
        HCK(hipGetLastError());
        const unsigned nb = (unsigned)std::max(1, std::min((N + kWavesPerBlock - 1) / kWavesPerBlock,
                                                           8 * ctx->cus));
        hipLaunchKernelGGL(covered_flags_tiled_kernel, dim3(nb), dim3(kBlock), 0, s,
                           ctx->xys.as<double2>(), ctx->off.as<int32_t>(), ctx->grid,
                           ctx->cdisk.as<DiskRec>(), N, ctx->flags_s.as<uint8_t>());
        HCK(hipGetLastError());
    }
    hipLaunchKernelGGL(scatter_flags_kernel, dim3(grid1d(M, 256)), dim3(256), 0, s,
                       ctx->flags_s.as<uint8_t>(), ctx->perm.as<uint32_t>(), M,
                       ctx->flags_o.as<uint8_t>());
    HCK(hipGetLastError());
}

int32_t mac_covered_flags_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                              uint8_t* flags_out)
{
    ABI_BEGIN
    int32_t rc = check_common(ctx, three_n, 0);
    if (rc) return rc;
    if (three_n > 0 && !circles) return fail(MAC_E_INVAL, "null circles");
    set_device(ctx);
    hipStream_t s = ctx->setup_stream;
    HCK(hipDeviceSynchronize());
    free_deferred(ctx);
    compute_flags(ctx, s, circles, (int)(three_n / 3));
    if (ctx->M > 0 && flags_out)
        HCK(hipMemcpyAsync(flags_out, ctx->flags_o.p, ctx->M, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    return MAC_OK;
    ABI_END
}

int32_t mac_remove_covered_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                               int64_t* kept_idx, int64_t* M_out)
{
    ABI_BEGIN
    int32_t rc = check_common(ctx, three_n, 0);
    if (rc) return rc;
    if (three_n > 0 && !circles) return fail(MAC_E_INVAL, "null circles");
    set_device(ctx);
    hipStream_t s = ctx->setup_stream;
    HCK(hipDeviceSynchronize());
    free_deferred(ctx);
    const int64_t M = ctx->M;
    compute_flags(ctx, s, circles, (int)(three_n / 3));
    int64_t kept = M;
    if (M > 0) {
        ctx->keep.reserve(M);
        hipLaunchKernelGGL(invert_flags_kernel, dim3(grid1d(M, 256)), dim3(256), 0, s,
                           ctx->flags_o.as<uint8_t>(), M, ctx->keep.as<uint8_t>());
        HCK(hipGetLastError());
        ctx->sel_count.reserve(sizeof(int64_t) * 4);
        const size_t b = sizeof(double) * M;
        ctx->cx.reserve(b);
        ctx->cy.reserve(b);
        ctx->cw.reserve(b);
        ctx->cidx.reserve(sizeof(int64_t) * M);
        size_t tb = 0, tb2 = 0;
        HCK(hipcub::DeviceSelect::Flagged(nullptr, tb, ctx->x.as<double>(), ctx->keep.as<uint8_t>(),
                                          ctx->cx.as<double>(), ctx->sel_count.as<int64_t>(), M, s));
        hipcub::CountingInputIterator<int64_t> it(0);
        HCK(hipcub::DeviceSelect::Flagged(nullptr, tb2, it, ctx->keep.as<uint8_t>(),
                                          ctx->cidx.as<int64_t>(), ctx->sel_count.as<int64_t>(), M,
                                          s));
        ctx->tmp.reserve(std::max(tb, tb2));
        HCK(hipcub::DeviceSelect::Flagged(ctx->tmp.p, tb, ctx->x.as<double>(), ctx->keep.as<uint8_t>(),
                                          ctx->cx.as<double>(), ctx->sel_count.as<int64_t>(), M, s));
        HCK(hipcub::DeviceSelect::Flagged(ctx->tmp.p, tb, ctx->y.as<double>(), ctx->keep.as<uint8_t>(),
                                          ctx->cy.as<double>(), ctx->sel_count.as<int64_t>(), M, s));
        HCK(hipcub::DeviceSelect::Flagged(ctx->tmp.p, tb, ctx->w.as<double>(), ctx->keep.as<uint8_t>(),
                                          ctx->cw.as<double>(), ctx->sel_count.as<int64_t>(), M, s));
        HCK(hipcub::DeviceSelect::Flagged(ctx->tmp.p, tb2, it, ctx->keep.as<uint8_t>(),
                                          ctx->cidx.as<int64_t>(), ctx->sel_count.as<int64_t>(), M,
                                          s));
        HCK(hipMemcpyAsync(&kept, ctx->sel_count.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        std::swap(ctx->x, ctx->cx);
        std::swap(ctx->y, ctx->cy);
        std::swap(ctx->w, ctx->cw);
        if (kept_idx && kept > 0)
            HCK(hipMemcpyAsync(kept_idx, ctx->cidx.p, sizeof(int64_t) * kept, hipMemcpyDeviceToHost,
                               s));
        ctx->M = kept;
        build_index(ctx, s);
    }
    if (M_out) *M_out = kept;
    return MAC_OK;
    ABI_END
}

// ------------------------------------------------------------------ high-interest regions

int32_t mac_set_regions(mac_ctx* ctx, const double* x_lb, const double* x_ub, const double* y_lb,
                        const double* y_ub, int32_t n_boxes, double w_high)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (n_boxes < 0 || n_boxes > kRegionsMax)
        return fail(MAC_E_INVAL, "n_boxes = " + std::to_string(n_boxes) + " outside [0, " +
                                     std::to_string(kRegionsMax) + "]");
    if (n_boxes > 0 && (!x_lb || !x_ub || !y_lb || !y_ub)) return fail(MAC_E_INVAL, "null bound array");
    set_device(ctx);
    hipStream_t s = ctx->setup_stream;
    HCK(hipDeviceSynchronize());
    free_deferred(ctx);
    if (n_boxes > 0) {
        ctx->rboxes.reserve(sizeof(double) * 4 * kRegionsMax);
        ctx->rcount.reserve(sizeof(unsigned long long) * (kRegionsMax + 1));
        double hb[4 * kRegionsMax];
        for (double& v : hb) v = NAN;
        for (int b = 0; b < n_boxes; ++b) {
            hb[b] = x_lb[b];
            hb[kRegionsMax + b] = x_ub[b];
            hb[2 * kRegionsMax + b] = y_lb[b];
            hb[3 * kRegionsMax + b] = y_ub[b];
        }
        HCK(hipMemcpyAsync(ctx->rboxes.p, hb, sizeof hb, hipMemcpyHostToDevice, s));
        HCK(hipMemsetAsync(ctx->rcount.p, 0, sizeof(unsigned long long) * (kRegionsMax + 1), s));
        HCK(hipStreamSynchronize(s));
        std::memcpy(ctx->h_boxes, hb, sizeof hb);
    }
    ctx->n_regions = n_boxes;
    ctx->reg_w_high = w_high;
    return MAC_OK;
    ABI_END
}

int32_t mac_regions_ingested(mac_ctx* ctx, int64_t* box_count, int64_t* any_count)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (ctx->n_regions == 0) return fail(MAC_E_INVAL, "no regions set (mac_set_regions)");
    set_device(ctx);
    hipStream_t s = ctx->setup_stream;
    unsigned long long h[kRegionsMax + 1];
    HCK(hipMemcpyAsync(h, ctx->rcount.p, sizeof h, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    if (box_count)
        for (int b = 0; b < ctx->n_regions; ++b) box_count[b] = (int64_t)h[b];
    if (any_count) *any_count = (int64_t)h[kRegionsMax];
    return MAC_OK;
    ABI_END
}

// The items of one stats call (k_regions.h RegItem): per box with lb < ub on both axes its tile
// range, split into bands of G rows and nch chunks per row so that an item holds about kRegChunk
// entries of a uniformly dense list and all items together stay under kRegItemCap.
static int regions_plan(const mac_ctx* ctx, RegItem* it)
{
    const Grid& g = ctx->grid;
    const int nb = ctx->n_regions;
    const double* B = ctx->h_boxes;
    int nvalid = 0;
    for (int b = 0; b < nb; ++b)
        nvalid += B[b] < B[kRegionsMax + b] && B[2 * kRegionsMax + b] < B[3 * kRegionsMax + b];
    const int capb = nvalid ? kRegItemCap / nvalid : 0;   // >= 1024
    int total = 0;
    for (int b = 0; b < nb; ++b) {
        RegItem& I = it[b];
        I = RegItem{0, 0, 0, -1, 1, 1, 0, total};
        if (!(B[b] < B[kRegionsMax + b] && B[2 * kRegionsMax + b] < B[3 * kRegionsMax + b])) continue;
        I.tx0 = tile_of(B[b], g.gx0, g.invS, g.nTx);
        I.tx1 = tile_of(B[kRegionsMax + b], g.gx0, g.invS, g.nTx);
        I.ty0 = tile_of(B[2 * kRegionsMax + b], g.gy0, g.invS, g.nTy);
        I.ty1 = tile_of(B[3 * kRegionsMax + b], g.gy0, g.invS, g.nTy);
        const int rows = I.ty1 - I.ty0 + 1;
        I.G = (rows + capb - 1) / capb;
        I.nrg = (rows + I.G - 1) / I.G;
        const double est = (double)ctx->M * ((double)(I.tx1 - I.tx0 + 1) / (double)g.nTx) *
                           ((double)I.G / (double)g.nTy);
        const double want = std::ceil(est / (double)kRegChunk);
        I.nch = (int)std::max(1.0, std::min(want, (double)(capb / I.nrg)));
        total += I.nrg * I.nch;
    }
    return total;
}

int32_t mac_region_stats_f64(mac_ctx* ctx, const double* circles, int64_t three_n, int64_t* box_count,
                             double* box_weight, int64_t* any_count, double* any_weight,
                             int64_t* covered_count, double* covered_weight)
{
    ABI_BEGIN
    int32_t rc = check_common(ctx, three_n, 0);
    if (rc) return rc;
    if (ctx->n_regions == 0) return fail(MAC_E_INVAL, "no regions set (mac_set_regions)");
    if (three_n > 0 && !circles) return fail(MAC_E_INVAL, "null circles");
    const int N = (int)(three_n / 3);
    if (N > kRegMaxDisks)
        return fail(MAC_E_INVAL, "mac_region_stats: N = " + std::to_string(N) + " > " +
                                     std::to_string(kRegMaxDisks) + " UAVs");
    const int nb = ctx->n_regions;
    std::vector<unsigned long long> hc(nb + 2, 0);
    std::vector<double> hw(nb + 2, 0.0);
    RegItem it[kRegionsMax];
    const int total = ctx->M > 0 ? regions_plan(ctx, it) : 0;
    if (total > 0) {
        set_device(ctx);
        hipStream_t s = ctx->setup_stream;
        HCK(hipDeviceSynchronize());
        free_deferred(ctx);
        ctx->ritems.reserve(sizeof(RegItem) * kRegionsMax);
        ctx->rpart.reserve(sizeof(RegPartial) * (size_t)total);
        ctx->rout.reserve((sizeof(unsigned long long) + sizeof(double)) * (kRegionsMax + 2));
        ctx->cdisk.reserve(sizeof(DiskRec) * std::max(N, 1));
        unsigned long long* d_oc = ctx->rout.as<unsigned long long>();
        double* d_ow = (double*)(d_oc + kRegionsMax + 2);
        HCK(hipMemcpyAsync(ctx->ritems.p, it, sizeof(RegItem) * nb, hipMemcpyHostToDevice, s));
        if (N > 0) {
            ctx->circ.reserve(sizeof(double) * 3 * N);
            HCK(hipMemcpyAsync(ctx->circ.p, circles, sizeof(double) * 3 * N, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(disk_prep_kernel, dim3(grid1d(N, 256)), dim3(256), 0, s,
                               matrix_src(ctx->circ.as<double>(), N), N, 1, ctx->cdisk.as<DiskRec>());
            HCK(hipGetLastError());
        }
        hipLaunchKernelGGL(region_stats_kernel, dim3(grid1d(total, kWavesPerBlock)), dim3(kBlock), 0, s,
                           ctx->xys.as<double2>(), ctx->ws.as<double>(), ctx->off.as<int32_t>(), ctx->grid,
                           ctx->rboxes.as<double>(), nb, ctx->ritems.as<RegItem>(), total,
                           ctx->cdisk.as<DiskRec>(), N, ctx->rpart.as<RegPartial>());
        HCK(hipGetLastError());
        hipLaunchKernelGGL(region_reduce_kernel, dim3(nb + 1), dim3(kBlock), 0, s,
                           ctx->rpart.as<RegPartial>(), ctx->ritems.as<RegItem>(), nb, total, d_oc, d_ow);
        HCK(hipGetLastError());
        HCK(hipMemcpyAsync(hc.data(), d_oc, sizeof(unsigned long long) * (nb + 2), hipMemcpyDeviceToHost, s));
        HCK(hipMemcpyAsync(hw.data(), d_ow, sizeof(double) * (nb + 2), hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
    }
    for (int b = 0; b < nb; ++b) {
        if (box_count) box_count[b] = (int64_t)hc[b];
        if (box_weight) box_weight[b] = hw[b];
    }
    if (any_count) *any_count = (int64_t)hc[nb];
    if (any_weight) *any_weight = hw[nb];
    if (covered_count) *covered_count = (int64_t)hc[nb + 1];
    if (covered_weight) *covered_weight = hw[nb + 1];
    return MAC_OK;
    ABI_END
}

// The single-candidate closure (k_closure.h): the candidates written by the host straight into the
// lane's fine-grained device buffer through the BAR (a large-BAR device; else pinned staging and a
// copy), one kernel (grid.y = the batch), each area from its own mapped slot (no copy either way,
// no stream synchronisation). AUTO / TILED walks, N <= kClosureMaxN; if a slot has not landed within 2 ms (a
// failed launch) a stream synchronisation reports it.
static constexpr int kClBatch = 64;   // concurrent mac_area_f64 calls evaluated by one launch
// slot reads spun with a pause before a reader starts yielding its CPU (MAXCOVER_CL_READSPIN overrides)
static const int kClReadSpin = [] {
    const char* e = std::getenv("MAXCOVER_CL_READSPIN");
    return e ? std::max(0, std::atoi(e)) : 64;
}();

static bool closure_path(const mac_ctx* ctx, int64_t three_n)
{
    return (ctx->algo == MAC_ALGO_AUTO || ctx->algo == MAC_ALGO_TILED) && three_n / 3 <= kClosureMaxN;
}

static const bool kClStats = [] {
    const char* e = std::getenv("MAXCOVER_CL_STATS");
    return e && *e == '1';
}();static void cl_add(std::atomic<int64_t>& a, std::chrono::steady_clock::duration d)
{
    a.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(d).count(), std::memory_order_relaxed);
}

// A launched batch of closure candidates: its lane (stream, staging, result slots) stays with the
// batch until every one of its callers has read its slot (the last returns the lane to the pool),
// so a later batch can neither overwrite a slot nor the staging before they are consumed.
struct ClBatch {
    Lane* L = nullptr;
    uint64_t seq = 0;
    std::atomic<int> readers{0};
};

// Write the B candidates into the lane's device buffer (through the BAR, or pinned staging and a
// copy) and launch one closure_kernel (grid.y = B) whose candidate b writes its area into the lane's mapped slot b under `seq`. Returns
// after enqueueing: the launching caller does not wait for the results.
static uint64_t closure_launch(mac_ctx* ctx, Lane* L, int64_t three_n, const double* const* cands, int B)
{
    const int N = (int)(three_n / 3);
    hipStream_t s = L->stream;
    const size_t one = sizeof(double) * (size_t)three_n;
    const auto t0 = std::chrono::steady_clock::now();
    const double* dc;
    bool bar = ctx->cl_bar.load(std::memory_order_relaxed);
    if (bar) {
        try {
            L->clv.reserve(one * kClBatch, true);
        } catch (const HipError&) {   // no fine-grained device memory to spare: the copy path from now on
            (void)hipGetLastError();
            ctx->cl_bar.store(false, std::memory_order_relaxed);
            bar = false;
        }
    }
    if (bar) {   // straight into device memory through the BAR; the fence drains the
                 // write-combining buffers before the launch's doorbell
        for (int b = 0; b < B; ++b) std::memcpy((char*)L->clv.p + one * b, cands[b], one);
        _mm_sfence();
        dc = L->clv.as<double>();
    } else {
        L->h_io.reserve(std::max<size_t>(one * B, 64));
        for (int b = 0; b < B; ++b) std::memcpy((char*)L->h_io.p + one * b, cands[b], one);
        L->cands.reserve(one * B);
        dc = L->cands.as<double>();
    }
    const auto t1 = std::chrono::steady_clock::now();
    L->area.reserve(sizeof(double) * B);
    L->cpart.reserve(sizeof(unsigned long long) * (size_t)N * B);
    // zero once; the last block of each candidate resets its words
    if (L->carrive.grow(sizeof(unsigned) * kClBatch)) HCK(hipMemsetAsync(L->carrive.p, 0, L->carrive.cap, s));
    if (L->ctot.grow(sizeof(uint64_t) * kClBatch)) HCK(hipMemsetAsync(L->ctot.p, 0, L->ctot.cap, s));
    if (!L->h_cl.p) {   // a 32-B slot per batch candidate
        L->h_cl.reserve(32 * kClBatch, hipHostMallocMapped | hipHostMallocCoherent);
        std::memset(L->h_cl.p, 0, 32 * kClBatch);
        void* dp = nullptr;
        HCK(hipHostGetDevicePointer(&dp, L->h_cl.p, 0));
        L->d_cl = (uint64_t*)dp;
    }
    const uint64_t seq = ++L->cl_seq;
    if (!bar) HCK(hipMemcpyAsync(L->cands.p, L->h_io.p, one * B, hipMemcpyHostToDevice, s));
    const int nwg = (N + kClosureDisksPerWG - 1) / kClosureDisksPerWG;   // a wave per disk
    int64_t ts_a = -1;
    uint64_t* ts = nullptr;
    if (ctx->profile) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (ctx->stamp_used + (int64_t)nwg * B <= ctx->stamp_cap) {
            ts_a = ctx->stamp_used;
            ctx->stamp_used += (int64_t)nwg * B;
            ts = ctx->stamps.as<uint64_t>() + 2 * ts_a;
        }
    }
    const ClosureOut co{L->cpart.as<unsigned long long>(), L->ctot.as<unsigned long long>(),
                        L->carrive.as<unsigned>(), L->area.as<double>(), L->d_cl, seq};
    hipLaunchKernelGGL(closure_kernel, dim3((unsigned)nwg, (unsigned)B), dim3(kBlock),
                       (uint32_t)closure_lds_bytes(N), s, ts, dc, N, ctx->grid,
                       ctx->xys.as<double2>(), ctx->ws.as<double>(), ctx->off.as<int32_t>(),
                       ctx->w_uniform ? 1 : 0, ctx->w0, co);
    HCK(hipGetLastError());
    if (ts) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        ctx->prof.push_back({ts_a, (int64_t)nwg * B, -1, 0, (int64_t)B, nullptr, MAC_ALGO_TILED});
    }
    if (kClStats) {
        const auto t2 = std::chrono::steady_clock::now();
        cl_add(ctx->cl_phase_ns[0], t1 - t0);
        cl_add(ctx->cl_phase_ns[1], t2 - t1);
    }
    return seq;
}

// Candidate b's area of a launched batch, from its mapped slot (spinning with pauses: the other
// callers' threads lead batches meanwhile); after 2 ms (a failed launch) the lane's stream is
// synchronised, which reports the error, then the slot or the device word is read.
static double closure_read(mac_ctx* ctx, ClBatch* bt, int b)
{
    const uint64_t* slot = (const uint64_t*)bt->L->h_cl.p + 4 * b;
    double a = 0.0;
    int64_t unused = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int spin = 0;; ++spin) {
        if (mirror_read(slot, bt->seq, &a, &unused)) return a;
        // past a short spin, yield the CPU between reads: under many concurrent callers the
        // threads launching the next batches need it more than the spinning readers (the call's
        // HIP enqueue time doubles when every CPU of the share spins)
        if (spin < kClReadSpin) __builtin_ia32_pause();
        else sched_yield();
        if ((spin & 255) == 255 &&
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 2.0)
            break;
    }
    set_device(ctx);
    HCK(hipStreamSynchronize(bt->L->stream));
    if (!mirror_read(slot, bt->seq, &a, &unused))
        HCK(hipMemcpy(&a, bt->L->area.as<double>() + b, sizeof(double), hipMemcpyDeviceToHost));
    return a;
}

// One caller is done with the batch; the last returns the lane (its stream holds nothing unread:
// every slot has landed, so the kernel that wrote them is ending, and later work on the stream is
// ordered after it).
static void closure_done(mac_ctx* ctx, ClBatch* bt)
{
    if (bt->readers.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        bt->L->last = bt->L->stream;
        ctx->lanes_free.push_back(bt->L);
    }
    delete bt;
}

// Concurrent callers (DirectSearch's threaded poll, src/TDM_STATIC_opt.jl:129: one objective call
// per trial point per thread) are combined: a caller queues its request; while fewer than
// kClLeaders batches are being launched, a caller whose request is still queued takes every queued
// request of the same size (up to kClBatch), launches them as one batch on a lane of its own and
// goes back to waiting for its own result like every other caller: no thread waits for a batch's
// results but the threads whose requests it holds, each on its own mapped slot, so the next batch
// can be formed and launched while earlier ones run (round 5's leaders waited for their whole batch
// before another could start). A lone caller launches its own request at once. Results per call are
// exactly the single-candidate kernel's (the batch dimension only selects the candidate).
#ifndef MAC_CL_LEADERS
#define MAC_CL_LEADERS 2
#endif
// batches being launched at once (MAXCOVER_CL_LEADERS overrides, for measurements)
static const int kClLeaders = [] {
    const char* e = std::getenv("MAXCOVER_CL_LEADERS");
    const int v = e ? std::atoi(e) : 0;
    return v >= 1 && v <= 16 ? v : MAC_CL_LEADERS;
}();
// pause iterations before a waiter sleeps on its futex (MAXCOVER_CL_SPIN overrides, for measurements)
static const int kClSpin = [] {
    const char* e = std::getenv("MAXCOVER_CL_SPIN");
    return e ? std::max(0, std::atoi(e)) : 64;
}();

static constexpr int kClGather = 0;        // pauses a would-be leader waits for every caller to queue (0: none)
// batches one thread launches in a row while requests are queued (MAXCOVER_CL_LEAD overrides): the
// launching thread is awake on a CPU, a queued caller woken to lead instead takes tens of
// microseconds to run; the cap bounds how long the leader's own call waits behind others' batches
static const int kClLead = [] {
    const char* e = std::getenv("MAXCOVER_CL_LEAD");
    const int v = e ? std::atoi(e) : 0;
    return v >= 1 ? v : 16;
}();

// Waiting while queued: a short spin, then a futex sleep (no CPU taken from the threads that lead
// batches) on the word of the request's generation, or 1 ms. A leader that launches generation g's
// batch bumps g's word and wakes ONE sleeper (a futex wake costs the waker microseconds per thread;
// the launching thread is the combiner's bottleneck); a thread woken with its request launched
// passes the wake on to the rest of its generation. A leader that frees a launch slot with requests
// still queued wakes one of them to lead.
static std::atomic<int>& cl_word(mac_ctx* ctx, uint32_t gen) { return ctx->cl_genw[gen & 63]; }

static void cl_wake(std::atomic<int>& w, int n)
{
    w.fetch_add(1, std::memory_order_seq_cst);
    syscall(SYS_futex, reinterpret_cast<int*>(&w), FUTEX_WAKE_PRIVATE, n, nullptr, nullptr, 0);
}

struct ClReq {
    const double* c;
    int64_t three_n;
    double* out;
    std::atomic<int> state{0};   // 0 queued, 1 taken by a batch, 2 failed, 3 launched (read the slot)
    std::atomic<int> released{0};   // 1 once the leader no longer touches the request (after its
                                    // futex wake): the owner's stack object may then go
    uint32_t gen = 0;            // the generation whose futex word this request sleeps on (cl_mu)
    std::chrono::steady_clock::time_point t_taken, t_handed;   // (MAXCOVER_CL_STATS=1)
    ClBatch* bt = nullptr;       // (state 3) the batch and this request's slot in it
    int b = 0;
    int32_t rc = MAC_OK;
    std::string err;
};

static void cl_wait(mac_ctx* ctx, ClReq& r, int spin)
{
    if (spin < kClSpin) {
        __builtin_ia32_pause();
        return;
    }
    uint32_t g = r.gen;   // (written by this thread only)
    if (r.state.load(std::memory_order_relaxed) == 0 && g != ctx->cl_gen.load(std::memory_order_relaxed)) {
        // still queued past an earlier take (a batch of another size): join the current generation
        std::lock_guard<std::mutex> lk(ctx->cl_mu);
        if (r.state.load(std::memory_order_relaxed) == 0) r.gen = ctx->cl_gen.load(std::memory_order_relaxed);
        g = r.gen;
    }
    std::atomic<int>& w = cl_word(ctx, g);
    const int v = w.load(std::memory_order_seq_cst);
    const int st = r.state.load(std::memory_order_seq_cst);
    if (st == 2 || st == 3) return;
    struct timespec ts{0, 1000000};
    syscall(SYS_futex, reinterpret_cast<int*>(&w), FUTEX_WAIT_PRIVATE, v, &ts, nullptr, 0);
    const int now = r.state.load(std::memory_order_acquire);
    if (now == 2 || now == 3) cl_wake(w, INT_MAX);   // the rest of the generation's sleepers
}

int32_t mac_area_f64(mac_ctx* ctx, const double* circles, int64_t three_n, double* area_out)
{
    ABI_BEGIN
    if (!area_out) return fail(MAC_E_INVAL, "null area_out");
    int32_t rc = check_common(ctx, three_n, 1);
    if (rc) return rc;
    if (!circles) return fail(MAC_E_INVAL, "null circles");
    if (!closure_path(ctx, three_n))
        return host_eval<double>(ctx, circles, three_n, 1, nullptr, 0.0, nullptr, nullptr, 1.0, area_out,
                                 nullptr, nullptr, nullptr);
    if (three_n == 0 || ctx->M == 0) {
        *area_out = 0.0;
        return MAC_OK;
    }
    ClReq r;
    r.c = circles;
    r.three_n = three_n;
    r.out = area_out;
    using clk = std::chrono::steady_clock;
    const auto tq = kClStats ? clk::now() : clk::time_point{};
    bool led = false;
    ctx->cl_active.fetch_add(1);
    {
        std::lock_guard<std::mutex> lk(ctx->cl_mu);
        r.gen = ctx->cl_gen.load(std::memory_order_relaxed);
        ctx->cl_q.push_back(&r);
    }
    // take every queued request of the front request's size (up to kClBatch) as a batch, if a
    // launch slot is free (under cl_mu)
    auto take = [&](std::vector<ClReq*>& batch, bool& mixed) {
        if (ctx->cl_busy >= kClLeaders || ctx->cl_q.empty()) return;
        ++ctx->cl_busy;
        ++ctx->cl_batches;
        const uint32_t g = ctx->cl_gen.fetch_add(1, std::memory_order_relaxed);   // requests queued from
                                                                                  // now on: the next batch's
        const int64_t tn = ctx->cl_q.front()->three_n;
        for (auto it = ctx->cl_q.begin(); it != ctx->cl_q.end() && (int)batch.size() < kClBatch;) {
            if ((*it)->three_n == tn) {
                if (kClStats) (*it)->t_taken = clk::now();
                (*it)->state.store(1, std::memory_order_relaxed);
                batch.push_back(*it);
                ++ctx->cl_reqs;
                ++ctx->cl_taken;
                it = ctx->cl_q.erase(it);
            } else {
                ++it;
            }
        }
        // a request of this generation left queued (another size, or past kClBatch) sleeps on the
        // same word: the batch's wake must then reach every sleeper, not one
        mixed = false;
        for (ClReq* q : ctx->cl_q) mixed |= q->gen == g;
    };
    std::vector<ClReq*> batch;
    bool mixed = false;
    for (int spin = 0, led_batches = 0;; ++spin) {
        const int st = r.state.load(std::memory_order_acquire);
        const bool mine = st == 2 || st == 3;   // this request is launched (or failed)
        if (mine && (batch.empty() || led_batches >= kClLead)) break;
        if (!mine && batch.empty() && ctx->cl_busy.load(std::memory_order_relaxed) < kClLeaders) {
            std::lock_guard<std::mutex> lk(ctx->cl_mu);
            // lead once every caller in the combiner has queued (the whole convoy in one launch),
            // or after a short wait
            const bool all_in = (int)ctx->cl_q.size() + ctx->cl_taken >= ctx->cl_active.load() ||
                                spin >= kClGather;
            if (r.state.load(std::memory_order_relaxed) == 0 && all_in) take(batch, mixed);
        }
        if (batch.empty()) {
            const int seen = r.state.load(std::memory_order_acquire);
            if (seen != 2 && seen != 3) cl_wait(ctx, r, spin);
            continue;
        }
        // lead: launch the batch, hand every request its slot; then, while requests are queued and
        // up to kClLead batches, lead again (this thread is awake on a CPU: a queued caller woken
        // to lead takes tens of microseconds to run under load), else wait for our own slot
        for (ClReq* q : batch) led |= q == &r;
        ++led_batches;
        const bool again = led_batches < kClLead;
        const auto tp = kClStats ? clk::now() : clk::time_point{};
        ClBatch* bt = new ClBatch();
        bt->readers.store((int)batch.size(), std::memory_order_relaxed);
        int32_t brc = MAC_OK;
        std::string msg;
        try {
            std::vector<const double*> cs(batch.size());
            for (size_t q = 0; q < batch.size(); ++q) cs[q] = batch[q]->c;
            set_device(ctx);
            bt->L = acquire_lane(ctx, nullptr);
            if (kClStats) cl_add(ctx->cl_phase_ns[3], clk::now() - tp);
            bt->seq = closure_launch(ctx, bt->L, batch[0]->three_n, cs.data(), (int)batch.size());
        } catch (const HipError& he) {
            brc = he.e == hipErrorOutOfMemory ? MAC_E_NOMEM : MAC_E_HIP;
            char buf[512];
            snprintf(buf, sizeof buf, "HIP error %d (%s) at maxcover.hip:%d in %s", (int)he.e,
                     hipGetErrorString(he.e), he.line, he.what);
            msg = buf;
        } catch (const std::bad_alloc&) {
            brc = MAC_E_NOMEM;
            msg = "host allocation failed";
        } catch (...) {
            brc = MAC_E_HIP;
            msg = "unexpected exception";
        }
        if (brc != MAC_OK) {   // nothing was launched: the lane back, the requests failed
            if (bt->L) {
                std::lock_guard<std::mutex> lk(ctx->mu);
                ctx->lanes_free.push_back(bt->L);
            }
            delete bt;
            bt = nullptr;
        }
        const auto th = kClStats ? clk::now() : clk::time_point{};
        std::vector<uint32_t> wake_gens;
        std::vector<ClReq*> handed;
        handed.swap(batch);
        const int wake_n = mixed ? INT_MAX : 1;
        {
            std::lock_guard<std::mutex> lk(ctx->cl_mu);
            --ctx->cl_busy;
            ctx->cl_taken -= (int)handed.size();
            if (again && brc == MAC_OK) {
                take(batch, mixed);   // the next batch, taken before this one's callers run
            } else {   // a queued request whose thread may lead the freed launch slot
                for (ClReq* q : ctx->cl_q)
                    if (q != &r) {
                        cl_wake(cl_word(ctx, q->gen), 1);
                        break;
                    }
            }
            // the generations of the handed-out requests (one, but for requests of another size
            // queued past an earlier take)
            for (ClReq* q : handed) wake_gens.push_back(q->gen);
        }
        for (size_t q = 0; q < handed.size(); ++q) {   // (a request lives until its released word reads 1)
            ClReq* rq = handed[q];
            rq->bt = bt;
            rq->b = (int)q;
            rq->rc = brc;
            rq->err = msg;
            if (kClStats) rq->t_handed = clk::now();
            rq->state.store(bt ? 3 : 2, std::memory_order_seq_cst);
            rq->released.store(1, std::memory_order_release);
        }
        // one sleeper per generation woken here; it wakes the others (cl_wait)
        std::sort(wake_gens.begin(), wake_gens.end());
        for (size_t q = 0; q < wake_gens.size(); ++q)
            if (q == 0 || wake_gens[q] != wake_gens[q - 1])
                cl_wake(cl_word(ctx, wake_gens[q]), wake_gens.front() == wake_gens.back() ? wake_n : INT_MAX);
        if (kClStats) cl_add(ctx->cl_phase_ns[2], clk::now() - th);
        spin = 0;
    }
    // the leader that launched this request may still be between its state store and its wake (the
    // futex word is this stack object): wait for its release, a few instructions away
    while (r.released.load(std::memory_order_acquire) == 0) __builtin_ia32_pause();
    const auto tl = kClStats ? clk::now() : clk::time_point{};
    if (r.state.load(std::memory_order_acquire) == 3) {
        try {
            *area_out = closure_read(ctx, r.bt, r.b);
        } catch (...) {
            closure_done(ctx, r.bt);
            ctx->cl_active.fetch_sub(1);
            throw;
        }
        closure_done(ctx, r.bt);
    }
    if (kClStats) {
        const auto te = clk::now();
        cl_add(ctx->cl_req_ns[0], r.t_taken - tq);
        cl_add(ctx->cl_req_ns[1], r.t_handed - r.t_taken);
        cl_add(ctx->cl_req_ns[2], tl - r.t_handed);
        cl_add(ctx->cl_req_ns[3], te - tl);
        cl_add(ctx->cl_req_ns[4], te - tq);
        ctx->cl_led.fetch_add(led, std::memory_order_relaxed);
    }
    ctx->cl_active.fetch_sub(1);
    if (r.rc) return fail(r.rc, r.err);
    return MAC_OK;
    ABI_END
}

int32_t mac_area_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                           double* area_out)
{
    ABI_BEGIN
    if (!area_out && K > 0) return fail(MAC_E_INVAL, "null area_out");
    return host_eval<double>(ctx, cands, three_n, K, nullptr, 0.0, nullptr, nullptr, 1.0, area_out,
                     nullptr, nullptr, nullptr);
    ABI_END
}

int32_t mac_objective_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                const double* r_max, double penalty, double* obj_out)
{
    ABI_BEGIN
    if (!obj_out && K > 0) return fail(MAC_E_INVAL, "null obj_out");
    if (!r_max && three_n > 0) return fail(MAC_E_INVAL, "null r_max");
    return host_eval<double>(ctx, cands, three_n, K, r_max, penalty, nullptr, nullptr, 1.0, nullptr,
                     obj_out, nullptr, nullptr);
    ABI_END
}

int32_t mac_poll_best_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                          const double* r_max, double penalty, const double* prev,
                          const double* d_lim, double tan_half_fov, double* obj_out,
                          double* best_obj, int64_t* best_idx)
{
    ABI_BEGIN
    if (!best_obj || !best_idx) return fail(MAC_E_INVAL, "null best output");
    if (!r_max && three_n > 0) return fail(MAC_E_INVAL, "null r_max");
    return host_eval<double>(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov, nullptr,
                     obj_out, best_obj, best_idx);
    ABI_END
}

int32_t mac_area_f32(mac_ctx* ctx, const float* circles, int64_t three_n, double* area_out)
{
    ABI_BEGIN
    if (!area_out) return fail(MAC_E_INVAL, "null area_out");
    return host_eval<float>(ctx, circles, three_n, 1, nullptr, 0.0, nullptr, nullptr, 1.0, area_out,
                            nullptr, nullptr, nullptr);
    ABI_END
}

int32_t mac_area_batch_f32(mac_ctx* ctx, const float* cands, int64_t three_n, int64_t K,
                           double* area_out)
{
    ABI_BEGIN
    if (!area_out && K > 0) return fail(MAC_E_INVAL, "null area_out");
    return host_eval<float>(ctx, cands, three_n, K, nullptr, 0.0, nullptr, nullptr, 1.0, area_out,
                            nullptr, nullptr, nullptr);
    ABI_END
}

int32_t mac_poll_best_f32(mac_ctx* ctx, const float* cands, int64_t three_n, int64_t K,
                          const double* r_max, double penalty, const float* prev,
                          const double* d_lim, double tan_half_fov, double* obj_out,
                          double* best_obj, int64_t* best_idx)
{
    ABI_BEGIN
    if (!best_obj || !best_idx) return fail(MAC_E_INVAL, "null best output");
    if (!r_max && three_n > 0) return fail(MAC_E_INVAL, "null r_max");
    return host_eval<float>(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov,
                            nullptr, obj_out, best_obj, best_idx);
    ABI_END
}

int32_t mac_area_batch_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                               double* d_area, void* stream)
{
    ABI_BEGIN
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (K == 0) return MAC_OK;
    if (!d_cands || !d_area) return fail(MAC_E_INVAL, "null device pointer");
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;   // NULL: HIP's null stream
    LaneGuard lg(ctx, s);
    const int N = (int)(three_n / 3);
    EvalReq rq;
    rq.src = matrix_src(d_cands, N);
    rq.N = N;
    rq.K = (int)K;
    rq.tiled = use_tiled(ctx, N, nullptr, three_n);
    rq.tan_half_fov = 1.0;
    rq.d_area = d_area;
    enqueue_eval(ctx, lg.lane, s, rq);
    return MAC_OK;
    ABI_END
}

// ---- per-disk attribution (k_bydisk.h): owned / exclusive weight per disk and the area, one launch
// per 65535 candidates (grid.y)

static int32_t by_disk_check(mac_ctx* ctx, const void* cands, int64_t three_n, int64_t K, const void* owned,
                             const void* excl, const void* area)
{
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (three_n / 3 > kClosureMaxN)
        return fail(MAC_E_INVAL, "mac_area_by_disk: N = " + std::to_string(three_n / 3) + " > " +
                                     std::to_string(kClosureMaxN) + " UAVs (the per-disk kernel's limit)");
    if (K == 0) return MAC_OK;
    if (!cands && three_n > 0) return fail(MAC_E_INVAL, "null candidates");
    if (!owned && !excl && !area) return fail(MAC_E_INVAL, "no output given (owned, exclusive and area all null)");
    return MAC_OK;
}

static void by_disk_enqueue(mac_ctx* ctx, Lane* L, hipStream_t s, const double* d_cands, int N, int64_t K,
                            double* d_owned, double* d_excl, double* d_area)
{
    constexpr int64_t kMaxY = 65535;   // grid.y
    const int64_t Kc = std::min(K, kMaxY);
    L->bdpart.reserve(sizeof(unsigned long long) * (size_t)N * (size_t)Kc);
    // zero once; the last workgroup of each candidate resets its counter
    if (L->bdarrive.grow(sizeof(unsigned) * (size_t)Kc)) HCK(hipMemsetAsync(L->bdarrive.p, 0, L->bdarrive.cap, s));
    const int nwg = (N + kClosureDisksPerWG - 1) / kClosureDisksPerWG;   // a wave per disk
    for (int64_t k0 = 0; k0 < K; k0 += kMaxY) {
        const int64_t B = std::min(kMaxY, K - k0);
        int64_t ts_a = -1;
        uint64_t* ts = nullptr;
        if (ctx->profile) {
            std::lock_guard<std::mutex> lk(ctx->mu);
            if (ctx->stamp_used + (int64_t)nwg * B <= ctx->stamp_cap) {
                ts_a = ctx->stamp_used;
                ctx->stamp_used += (int64_t)nwg * B;
                ts = ctx->stamps.as<uint64_t>() + 2 * ts_a;
            }
        }
        const size_t o = (size_t)k0 * (size_t)N;
        const ByDiskOut bo{d_owned ? d_owned + o : nullptr, d_excl ? d_excl + o : nullptr,
                           d_area ? d_area + k0 : nullptr, L->bdpart.as<unsigned long long>(),
                           L->bdarrive.as<unsigned>()};
        hipLaunchKernelGGL(by_disk_kernel, dim3((unsigned)nwg, (unsigned)B), dim3(kBlock),
                           (uint32_t)closure_lds_bytes(N), s, ts, d_cands + 3 * o, N, ctx->grid,
                           ctx->xys.as<double2>(), ctx->ws.as<double>(), ctx->off.as<int32_t>(),
                           ctx->w_uniform ? 1 : 0, ctx->w0, bo);
        HCK(hipGetLastError());
        if (ts) {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->prof.push_back({ts_a, (int64_t)nwg * B, -1, 0, B, nullptr, MAC_ALGO_TILED});
        }
    }
}

// Host-pointer calls: upload, one launch, one download, the lane's stream synchronised.
static int32_t by_disk_host(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K, double* owned_out,
                            double* excl_out, double* area_out)
{
    int32_t rc = by_disk_check(ctx, cands, three_n, K, owned_out, excl_out, area_out);
    if (rc || K == 0) return rc;
    const int N = (int)(three_n / 3);
    const size_t nk = (size_t)N * (size_t)K;
    if (three_n == 0 || ctx->M == 0) {   // nothing to cover, or nothing covering
        if (owned_out) std::fill(owned_out, owned_out + nk, 0.0);
        if (excl_out) std::fill(excl_out, excl_out + nk, 0.0);
        if (area_out) std::fill(area_out, area_out + K, 0.0);
        return MAC_OK;
    }
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t in_bytes = sizeof(double) * (size_t)three_n * (size_t)K;
    const size_t nO = owned_out ? nk : 0, nX = excl_out ? nk : 0, nA = area_out ? (size_t)K : 0;
    const size_t out_bytes = sizeof(double) * (nO + nX + nA);
    L->cands.reserve(in_bytes);
    L->bdout.reserve(out_bytes);   // [owned][exclusive][area], one download
    double* d_o = L->bdout.as<double>();
    double* d_x = d_o + nO;
    double* d_a = d_x + nX;
    const bool staged = std::max(in_bytes, out_bytes) <= ((size_t)64 << 20);
    if (staged) {
        L->h_io.reserve(std::max<size_t>(std::max(in_bytes, out_bytes), 64));
        staged_upload(cands, L->h_io.p, L->cands.p, in_bytes, s);
    } else {
        HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    }
    by_disk_enqueue(ctx, L, s, L->cands.as<double>(), N, K, nO ? d_o : nullptr, nX ? d_x : nullptr,
                    nA ? d_a : nullptr);
    if (staged) {   // (the upload has completed before the kernel ran: the staging is free again)
        HCK(hipMemcpyAsync(L->h_io.p, d_o, out_bytes, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        const double* h = (const double*)L->h_io.p;
        if (nO) std::memcpy(owned_out, h, sizeof(double) * nO);
        if (nX) std::memcpy(excl_out, h + nO, sizeof(double) * nX);
        if (nA) std::memcpy(area_out, h + nO + nX, sizeof(double) * nA);
    } else {
        if (nO) HCK(hipMemcpyAsync(owned_out, d_o, sizeof(double) * nO, hipMemcpyDeviceToHost, s));
        if (nX) HCK(hipMemcpyAsync(excl_out, d_x, sizeof(double) * nX, hipMemcpyDeviceToHost, s));
        if (nA) HCK(hipMemcpyAsync(area_out, d_a, sizeof(double) * nA, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
    }
    return MAC_OK;
}

int32_t mac_area_by_disk_f64(mac_ctx* ctx, const double* circles, int64_t three_n, double* owned_out,
                             double* exclusive_out, double* area_out)
{
    ABI_BEGIN
    return by_disk_host(ctx, circles, three_n, 1, owned_out, exclusive_out, area_out);
    ABI_END
}

int32_t mac_area_by_disk_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                   double* owned_out, double* exclusive_out, double* area_out)
{
    ABI_BEGIN
    return by_disk_host(ctx, cands, three_n, K, owned_out, exclusive_out, area_out);
    ABI_END
}

int32_t mac_area_by_disk_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                                 double* d_owned, double* d_exclusive, double* d_area, void* stream)
{
    ABI_BEGIN
    int32_t rc = by_disk_check(ctx, d_cands, three_n, K, d_owned, d_exclusive, d_area);
    if (rc || K == 0) return rc;
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;   // NULL: HIP's null stream
    const int N = (int)(three_n / 3);
    const size_t nk = sizeof(double) * (size_t)N * (size_t)K;
    if (three_n == 0 || ctx->M == 0) {
        if (d_owned && nk) HCK(hipMemsetAsync(d_owned, 0, nk, s));
        if (d_exclusive && nk) HCK(hipMemsetAsync(d_exclusive, 0, nk, s));
        if (d_area) HCK(hipMemsetAsync(d_area, 0, sizeof(double) * (size_t)K, s));
        return MAC_OK;
    }
    LaneGuard lg(ctx, s);
    by_disk_enqueue(ctx, lg.lane, s, d_cands, N, K, d_owned, d_exclusive, d_area);
    return MAC_OK;
    ABI_END
}

}  // extern "C" (the template below has C++ linkage)

// The argument checks of a device poll (every failure a device poll can report before it
// enqueues anything but a HIP error): an armed poll runs them before its stream wait goes in.
static int32_t poll_dev_check(mac_ctx* ctx, const void* d_cands, int64_t three_n, int64_t K,
                              const void* d_prev, const double* d_dlim, const void* d_best)
{
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (!d_best) return fail(MAC_E_INVAL, "null d_best");
    if (K > 0 && !d_cands) return fail(MAC_E_INVAL, "null d_cands");
    if (d_prev && !d_dlim) return fail(MAC_E_INVAL, "d_prev given without d_dlim");
    return MAC_OK;
}

// d_best's mapped result slot {obj, idx, seq, check} (k_final.h): its own, else the least recently
// used one (a fetch still waiting on a reassigned slot sees another seq and falls back to the
// stream + copy). Returns the slot's device address and the seq the next write carries.
static uint64_t* assign_mirror(mac_ctx* ctx, const void* d_best, uint64_t* seq)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->d_mirror) {
        const size_t b = sizeof(uint64_t) * 4 * mac_ctx::kMirrorSlots;
        ctx->h_mirror.reserve(b, hipHostMallocMapped | hipHostMallocCoherent);
        std::memset(ctx->h_mirror.p, 0, b);
        void* dp = nullptr;
        HCK(hipHostGetDevicePointer(&dp, ctx->h_mirror.p, 0));
        ctx->d_mirror = (uint64_t*)dp;
    }
    int q = 0;
    for (int j = 0; j < mac_ctx::kMirrorSlots; ++j) {
        if (ctx->mirror_key[j] == d_best) {
            q = j;
            break;
        }
        if (ctx->mirror_used[j] < ctx->mirror_used[q]) q = j;
    }
    ctx->mirror_key[q] = d_best;
    ctx->mirror_used[q] = ++ctx->mirror_clock;
    *seq = ctx->mirror_want[q] = ++ctx->mirror_seq;
    return ctx->d_mirror + 4 * q;
}

template <class T>
static int32_t poll_best_dev(mac_ctx* ctx, const T* d_cands_in, int64_t three_n, int64_t K,
                             const double* d_rmax, double penalty, const T* d_prev_in,
                             const double* d_dlim, double tan_half_fov, int64_t idx_base,
                             double* d_obj, void* d_best, void* stream, const ConsArgs* cons = nullptr)
{
    if (ctx && ctx->host_stats) t_poll_entry = std::chrono::steady_clock::now();
    constexpr bool f32 = std::is_same<T, float>::value;
    int32_t rc = poll_dev_check(ctx, d_cands_in, three_n, K, d_prev_in, d_dlim, d_best);
    if (rc) return rc;
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;   // NULL: HIP's null stream
    LaneGuard lg(ctx, s);
    Lane* L = lg.lane;
    const int N = (int)(three_n / 3);
    const double* d_cands;
    const double* d_prev;
    if constexpr (f32) {   // widened into the lane's scratch, stream-ordered before the chain
        L->cands.reserve(sizeof(double) * (size_t)std::max<int64_t>(three_n * K, 1));
        widen_async(d_cands_in, three_n * K, L->cands.as<double>(), s);
        d_cands = L->cands.as<double>();
        d_prev = nullptr;
        if (d_prev_in) {
            L->prev.reserve(sizeof(double) * (size_t)std::max<int64_t>(three_n, 1));
            widen_async(d_prev_in, three_n, L->prev.as<double>(), s);
            d_prev = L->prev.as<double>();
        }
    } else {
        d_cands = d_cands_in;
        d_prev = d_prev_in;
    }
    if (K == 0) {
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            for (int q = 0; q < mac_ctx::kMirrorSlots; ++q)
                if (ctx->mirror_key[q] == d_best) ctx->mirror_key[q] = nullptr;   // fetch: copy
        }
        double hb[2] = {INFINITY, __builtin_bit_cast(double, (int64_t)-1)};
        L->best.reserve(16);
        HCK(hipMemcpyAsync(d_best, hb, 16, hipMemcpyHostToDevice, s));
        HCK(hipStreamSynchronize(s));
        return MAC_OK;
    }
    // cons3: the raw d_lim goes down the chain; the kernels that read it threshold it once per
    // UAV (k_prep.h pen_threshold)
    const double* d_dlimT = nullptr;
    double* d_o = d_obj;
    if (!d_o) {
        L->obj.reserve(sizeof(double) * K);
        d_o = L->obj.as<double>();
    }
    if (K > 1 && !t_defer_free && !ctx->route_seeded.exchange(true)) {   // (seed_route)
        std::vector<double> x0((size_t)three_n);
        HCK(hipMemcpyAsync(x0.data(), d_cands, sizeof(double) * (size_t)three_n, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        seed_route(ctx, x0.data(), N);
    }
    uint64_t seq = 0;
    uint64_t* d_mirror = assign_mirror(ctx, d_best, &seq);
    EvalReq rq;
    rq.src = matrix_src(d_cands, N);
    rq.N = N;
    rq.K = (int)K;
    rq.tiled = use_tiled(ctx, N, nullptr, three_n);
    rq.d_rmax = d_rmax;
    rq.penalty = penalty;
    rq.d_prev = d_prev;
    rq.d_dlimT = d_dlimT;
    rq.d_dlim_raw = d_dlim;
    rq.tan_half_fov = tan_half_fov;
    rq.d_obj = d_o;
    if (cons) {
        // the masked poll (mac_poll_best_cons_dev_f64): the mask, the chain unchanged into the lane's
        // own best (no slot), then the masked argmin into d_o (in place), d_best and its slot
        L->cmask.reserve((size_t)K);
        L->cbest.reserve(16);
        cons_mask_enqueue(s, d_cands, N, K, *cons, L->cmask.as<uint8_t>());
        rq.d_best = L->cbest.as<double>();
        enqueue_eval(ctx, L, s, rq);
        cons_argmin_enqueue(s, d_o, L->cmask.as<uint8_t>(), K, idx_base, d_best, d_mirror, seq);
        return MAC_OK;
    }
    rq.d_best = (double*)d_best;
    rq.idx_base = idx_base;
    rq.d_mirror = d_mirror;
    rq.mirror_seq = seq;
    enqueue_eval(ctx, L, s, rq);
    return MAC_OK;
}

extern "C" {

int32_t mac_poll_best_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                              const double* d_rmax, double penalty, const double* d_prev,
                              const double* d_dlim, double tan_half_fov, int64_t idx_base,
                              double* d_obj, void* d_best, void* stream)
{
    ABI_BEGIN
    return poll_best_dev<double>(ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim,
                                 tan_half_fov, idx_base, d_obj, d_best, stream);
    ABI_END
}

// Release tickets up to t (the doorbell's value), then every voided ticket that follows
// (guarded by mu).
static void release_tickets(mac_ctx* ctx, uint64_t t)
{
    if (t > ctx->fired) ctx->fired = t;
    for (bool more = true; more;) {
        more = false;
        for (size_t q = 0; q < ctx->voided.size(); ++q)
            if (ctx->voided[q] <= ctx->fired + 1) {
                ctx->fired = std::max(ctx->fired, ctx->voided[q]);
                ctx->voided.erase(ctx->voided.begin() + (long)q);
                more = true;
                break;
            }
    }
    __atomic_store_n(ctx->doorbell, ctx->fired, __ATOMIC_RELEASE);
}

int32_t mac_poll_arm_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                             const double* d_rmax, double penalty, const double* d_prev,
                             const double* d_dlim, double tan_half_fov, int64_t idx_base,
                             double* d_obj, void* d_best, void* stream, uint64_t* ticket)
{
    ABI_BEGIN
    if (!ctx || !ticket) return fail(MAC_E_INVAL, "null context / ticket");
    if (K <= 0) return fail(MAC_E_INVAL, "an armed poll needs K > 0");   // (K = 0 synchronises)
    // every argument failure is reported before the wait goes into the stream
    int32_t rc = poll_dev_check(ctx, d_cands, three_n, K, d_prev, d_dlim, d_best);
    if (rc) return rc;
    // not on HIP's null stream: until the fire, a wait there would block every blocking-stream
    // operation of the process (the library's own synchronous copies, torch's .item() / .cpu())
    if (!stream) return fail(MAC_E_INVAL, "an armed poll needs a stream (not HIP's null stream)");
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;
    uint64_t t = 0;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        if (!ctx->doorbell) {
            int ok = 0;
            HCK(hipDeviceGetAttribute(&ok, hipDeviceAttributeCanUseStreamWaitValue, ctx->device));
            if (!ok) return fail(MAC_E_HIP, "the device cannot wait on stream values");
            // coherent host memory: the host rings it with a plain atomic store, the stream's
            // wait polls it (a signal-memory doorbell would need the HSA signal API to wake it)
            void* p = nullptr;
            HCK(hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
            ctx->doorbell = (uint64_t*)p;
            __atomic_store_n(ctx->doorbell, (uint64_t)0, __ATOMIC_RELEASE);
            ctx->armed = ctx->fired = 0;
        }
        t = ++ctx->armed;
        bool found = false;
        for (auto& a : ctx->armed_on)
            if (a.first == s) {
                a.second = t;
                found = true;
            }
        if (!found) ctx->armed_on.push_back({s, t});
    }
    *ticket = t;
    // buffers the poll grows are not freed here (hipFree would wait for the device, which waits
    // for this ticket): they are kept until the next device synchronisation
    std::vector<std::pair<void*, bool>> defer;
    t_defer_free = &defer;
    bool ok = false;
    try {
        HCK(hipStreamWaitValue64(s, ctx->doorbell, t, hipStreamWaitValueGte, ~(uint64_t)0));
        rc = poll_best_dev<double>(ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim,
                                   tan_half_fov, idx_base, d_obj, d_best, stream);
        ok = rc == MAC_OK;
    } catch (...) {
        rc = -1;
    }
    t_defer_free = nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->deferred.insert(ctx->deferred.end(), defer.begin(), defer.end());
    if (!ok) {
        // the poll did not go in: only its own ticket is released (now if every earlier one is,
        // else together with the last of them), never an earlier armed poll's
        if (t == ctx->fired + 1)
            release_tickets(ctx, t);
        else
            ctx->voided.push_back(t);
        if (rc < 0) return fail(MAC_E_HIP, "arming the poll failed");
    }
    return rc;
    ABI_END
}

int32_t mac_poll_fire(mac_ctx* ctx, uint64_t ticket)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->doorbell || ticket > ctx->armed) return fail(MAC_E_INVAL, "ticket was not armed");
    if (ticket > ctx->fired) release_tickets(ctx, ticket);
    return MAC_OK;
}

int32_t mac_poll_best_dev_f32(mac_ctx* ctx, const float* d_cands, int64_t three_n, int64_t K,
                              const double* d_rmax, double penalty, const float* d_prev,
                              const double* d_dlim, double tan_half_fov, int64_t idx_base,
                              double* d_obj, void* d_best, void* stream)
{
    ABI_BEGIN
    return poll_best_dev<float>(ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim,
                                tan_half_fov, idx_base, d_obj, d_best, stream);
    ABI_END
}

// ---- swarm constraints (k_cons.h; include/maxcover.h mac_cons)

// The mask calls' argument checks. The point list is not read: no MAC_E_NOPOINTS.
static int32_t cons_check(mac_ctx* ctx, const void* cands, int64_t three_n, int64_t K, const void* out)
{
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (three_n < 0 || K < 0) return fail(MAC_E_INVAL, "negative size");
    if (three_n % 3 != 0)
        return fail(MAC_E_SIZE, "InexactError: Int64(" + std::to_string(three_n) + "/3)");
    if (three_n / 3 > kConsMaxN)
        return fail(MAC_E_INVAL, "mac_cons: N = " + std::to_string(three_n / 3) + " > " + std::to_string(kConsMaxN) +
                                     " UAVs (the constraint kernel's limit)");
    if (K > (int64_t)1 << 30) return fail(MAC_E_INVAL, "K too large");
    if (K == 0) return MAC_OK;
    if (!cands && three_n > 0) return fail(MAC_E_INVAL, "null candidates");
    if (!out) return fail(MAC_E_INVAL, "null feasibility output");
    return MAC_OK;
}

int32_t mac_cons_mask_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K, const mac_cons* cons,
                          uint8_t* feasible_out)
{
    ABI_BEGIN
    int32_t rc = cons_check(ctx, cands, three_n, K, feasible_out);
    if (rc || K == 0) return rc;
    ConsArgs a;
    if (!cons_active(cons, &a) || three_n == 0) {   // nothing on, or no UAV to violate anything
        std::memset(feasible_out, 1, (size_t)K);
        return MAC_OK;
    }
    const int N = (int)(three_n / 3);
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t in_bytes = sizeof(double) * (size_t)three_n * (size_t)K;
    L->cands.reserve(in_bytes);
    L->cmask.reserve((size_t)K);
    const bool staged = in_bytes <= ((size_t)64 << 20);
    if (staged) {
        L->h_io.reserve(std::max<size_t>(in_bytes, 64));
        staged_upload(cands, L->h_io.p, L->cands.p, in_bytes, s);
    } else {
        HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    }
    cons_mask_enqueue(s, L->cands.as<double>(), N, K, a, L->cmask.as<uint8_t>());
    if (staged && (size_t)K <= L->h_io.cap) {   // (the upload has completed before the kernel ran)
        HCK(hipMemcpyAsync(L->h_io.p, L->cmask.p, (size_t)K, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        std::memcpy(feasible_out, L->h_io.p, (size_t)K);
    } else {
        HCK(hipMemcpyAsync(feasible_out, L->cmask.p, (size_t)K, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
    }
    return MAC_OK;
    ABI_END
}

int32_t mac_cons_mask_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                              const mac_cons* cons, uint8_t* d_feasible, void* stream)
{
    ABI_BEGIN
    int32_t rc = cons_check(ctx, d_cands, three_n, K, d_feasible);
    if (rc || K == 0) return rc;
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;   // NULL: HIP's null stream
    ConsArgs a;
    if (!cons_active(cons, &a) || three_n == 0) {
        HCK(hipMemsetAsync(d_feasible, 1, (size_t)K, s));
        return MAC_OK;
    }
    cons_mask_enqueue(s, d_cands, (int)(three_n / 3), K, a, d_feasible);
    return MAC_OK;
    ABI_END
}

int32_t mac_poll_best_cons_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                               const double* r_max, double penalty, const double* prev,
                               const double* d_lim, double tan_half_fov, double* obj_out,
                               double* best_obj, int64_t* best_idx, const mac_cons* cons)
{
    ConsArgs a;
    if (!cons_active(cons, &a))   // nothing on: the plain call, untouched
        return mac_poll_best_f64(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov, obj_out,
                                 best_obj, best_idx);
    ABI_BEGIN
    if (!best_obj || !best_idx) return fail(MAC_E_INVAL, "null best output");
    if (!r_max && three_n > 0) return fail(MAC_E_INVAL, "null r_max");
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (three_n / 3 > kConsMaxN)
        return fail(MAC_E_INVAL, "mac_poll_best_cons: N = " + std::to_string(three_n / 3) + " > " +
                                     std::to_string(kConsMaxN) + " UAVs (the constraint kernel's limit)");
    return host_eval<double>(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov, nullptr,
                             obj_out, best_obj, best_idx, &a);
    ABI_END
}

int32_t mac_poll_best_cons_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                                   const double* d_rmax, double penalty, const double* d_prev,
                                   const double* d_dlim, double tan_half_fov, int64_t idx_base,
                                   double* d_obj, void* d_best, void* stream, const mac_cons* cons)
{
    ConsArgs a;
    if (!cons_active(cons, &a) || K == 0)   // nothing on (or nothing to mask): the plain call, untouched
        return mac_poll_best_dev_f64(ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim, tan_half_fov,
                                     idx_base, d_obj, d_best, stream);
    ABI_BEGIN
    int32_t rc = poll_dev_check(ctx, d_cands, three_n, K, d_prev, d_dlim, d_best);
    if (rc) return rc;
    if (three_n / 3 > kConsMaxN)
        return fail(MAC_E_INVAL, "mac_poll_best_cons_dev: N = " + std::to_string(three_n / 3) + " > " +
                                     std::to_string(kConsMaxN) + " UAVs (the constraint kernel's limit)");
    if ((uintptr_t)d_best & 7) return fail(MAC_E_INVAL, "d_best not 8-byte aligned");
    return poll_best_dev<double>(ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim, tan_half_fov,
                                 idx_base, d_obj, d_best, stream, &a);
    ABI_END
}

// ---- target-motion constraints (k_cons.h; include/maxcover.h mac_motion)

void mac_motion_thresholds(double speed_prev, double a_max, double* q_hi, double* q_lo)
{
    double hi, lo;
    motion_thresholds(speed_prev, a_max, &hi, &lo);
    if (q_hi) *q_hi = hi;
    if (q_lo) *q_lo = lo;
}

int32_t mac_cons_mask_motion_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                 const mac_cons* cons, uint8_t* feasible_out, const mac_motion* motion)
{
    bool mc, ms, ma;
    if (!motion_on(motion, &mc, &ms, &ma))   // nothing on: the plain call, untouched
        return mac_cons_mask_f64(ctx, cands, three_n, K, cons, feasible_out);
    ABI_BEGIN
    int32_t rc = cons_check(ctx, cands, three_n, K, feasible_out);
    if (rc || K == 0) return rc;
    if (three_n == 0) {   // no UAV to violate anything
        std::memset(feasible_out, 1, (size_t)K);
        return MAC_OK;
    }
    ConsArgs a{};
    cons_active(cons, &a);
    const int N = (int)(three_n / 3);
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t in_bytes = sizeof(double) * (size_t)three_n * (size_t)K;
    L->cands.reserve(in_bytes);
    L->cmask.reserve((size_t)K);
    const MotionArgs mot = motion_upload(L, s, N, motion);
    const bool staged = in_bytes <= ((size_t)64 << 20);
    if (staged) {
        L->h_io.reserve(std::max<size_t>(in_bytes, 64));
        staged_upload(cands, L->h_io.p, L->cands.p, in_bytes, s);
    } else {
        HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    }
    cons_mask_enqueue(s, L->cands.as<double>(), N, K, a, L->cmask.as<uint8_t>(), &mot);
    if (staged && (size_t)K <= L->h_io.cap) {   // (the upload has completed before the kernel ran)
        HCK(hipMemcpyAsync(L->h_io.p, L->cmask.p, (size_t)K, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
        std::memcpy(feasible_out, L->h_io.p, (size_t)K);
    } else {
        HCK(hipMemcpyAsync(feasible_out, L->cmask.p, (size_t)K, hipMemcpyDeviceToHost, s));
        HCK(hipStreamSynchronize(s));
    }
    return MAC_OK;
    ABI_END
}

int32_t mac_poll_best_motion_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                 const double* r_max, double penalty, const double* prev,
                                 const double* d_lim, double tan_half_fov, double* obj_out,
                                 double* best_obj, int64_t* best_idx, const mac_cons* cons,
                                 const mac_motion* motion)
{
    bool mc, ms, ma;
    if (!motion_on(motion, &mc, &ms, &ma))   // nothing on: the _cons call, untouched
        return mac_poll_best_cons_f64(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov, obj_out,
                                      best_obj, best_idx, cons);
    ABI_BEGIN
    if (!best_obj || !best_idx) return fail(MAC_E_INVAL, "null best output");
    if (!r_max && three_n > 0) return fail(MAC_E_INVAL, "null r_max");
    int32_t rc = check_common(ctx, three_n, K);
    if (rc) return rc;
    if (three_n / 3 > kConsMaxN)
        return fail(MAC_E_INVAL, "mac_poll_best_motion: N = " + std::to_string(three_n / 3) + " > " +
                                     std::to_string(kConsMaxN) + " UAVs (the constraint kernel's limit)");
    ConsArgs a{};
    cons_active(cons, &a);
    return host_eval<double>(ctx, cands, three_n, K, r_max, penalty, prev, d_lim, tan_half_fov, nullptr,
                             obj_out, best_obj, best_idx, &a, motion);
    ABI_END
}

// ---- constraint verdicts (k_cons.h cons_explain; include/maxcover.h mac_verdict)

static_assert(sizeof(mac_verdict) == sizeof(Verdict) && MAC_VERDICT_KINDS == kVerdictKinds, "mac_verdict is Verdict");

// The explain launches' arguments from what a call or a stepper has on: the swarm constraints (a: all
// off when none), the motion arrays as uploaded (null: none) and cons3's device inputs (null: off).
static ExplainArgs explain_args(const ConsArgs& a, const MotionArgs* mot, const double* d_prev,
                                const double* d_dlimT, double tan_half_fov)
{
    ExplainArgs xa{};
    xa.a = a;
    if (mot) xa.m = *mot;
    xa.pa = PenArgs{nullptr, d_prev, d_dlimT, nullptr, tan_half_fov};
    return xa;
}

int32_t mac_cons_explain_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K, const double* prev,
                             const double* d_lim, double tan_half_fov, const mac_cons* cons,
                             const mac_motion* motion, mac_verdict* out)
{
    ABI_BEGIN
    int32_t rc = cons_check(ctx, cands, three_n, K, out);
    if (rc) return rc;
    if (prev && !d_lim) return fail(MAC_E_INVAL, "prev given without d_lim");
    if (K == 0) return MAC_OK;
    ConsArgs a{};
    const bool has_cons = cons_active(cons, &a);
    if (!has_cons) a = cons_args(0.0, NAN, NAN);   // (everything off, T and dcut defined)
    bool mc, ms, ma;
    const bool has_mot = motion_on(motion, &mc, &ms, &ma);
    if (three_n == 0 || (!has_cons && !has_mot && !prev)) {   // no UAV, or nothing on: nothing rejects
        for (int64_t k = 0; k < K; ++k) {
            std::memset(&out[k], 0, sizeof(mac_verdict));
            for (int q = 0; q < MAC_VERDICT_KINDS; ++q) out[k].first_uav[q] = -1;
        }
        return MAC_OK;
    }
    const int N = (int)(three_n / 3);
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t in_bytes = sizeof(double) * (size_t)three_n * (size_t)K;
    const size_t out_bytes = sizeof(Verdict) * (size_t)K;
    L->cands.reserve(in_bytes);
    L->verdict.reserve(out_bytes);
    MotionArgs mot{};
    if (has_mot) mot = motion_upload(L, s, N, motion);
    if (prev) cons3_upload(L, s, N, prev, d_lim);
    const ExplainArgs xa = explain_args(a, has_mot ? &mot : nullptr, prev ? L->prev.as<double>() : nullptr,
                                        prev ? L->dlim.as<double>() : nullptr, tan_half_fov);
    const bool staged = in_bytes <= ((size_t)64 << 20);
    if (staged) {
        L->h_io.reserve(std::max<size_t>(in_bytes, 64));
        staged_upload(cands, L->h_io.p, L->cands.p, in_bytes, s);
    } else {
        HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    }
    constexpr int64_t kMaxWG = (int64_t)1 << 23;   // workgroups per launch (2^31 threads)
    const int S = cons_slots(N);
    const bool sep = a.sep != 0;
    for (int64_t k0 = 0; k0 < K; k0 += kMaxWG) {
        const int64_t B = std::min(kMaxWG, K - k0);
        hipLaunchKernelGGL(explain_kern(S, sep), dim3((unsigned)B), dim3(kConsBlock), explain_lds(S, sep), s,
                           L->cands.as<double>() + (size_t)k0 * (size_t)three_n, N, xa, L->verdict.as<Verdict>() + k0);
        HCK(hipGetLastError());
    }
    // (pageable destination: the copy stages through the runtime and has landed at the synchronisation)
    HCK(hipMemcpyAsync(out, L->verdict.p, out_bytes, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    return MAC_OK;
    ABI_END
}

// The context's tally for a stepper that begins with MAC_OPT_VERDICTS on: allocated and zeroed once.
static unsigned long long* verdict_tally(mac_ctx* ctx)
{
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->vtally.p) {
        ctx->vtally.reserve(sizeof(unsigned long long) * kVerdictTally);
        // (complete before any lane's launch adds to it: the lanes' streams do not wait for the null stream)
        HCK(hipMemsetAsync(ctx->vtally.p, 0, sizeof(unsigned long long) * kVerdictTally, nullptr));
        HCK(hipStreamSynchronize(nullptr));
    }
    return ctx->vtally.as<unsigned long long>();
}

int32_t mac_verdict_read(mac_ctx* ctx, int64_t* candidates, int64_t* rejected_any, int64_t* rejected_by,
                         int64_t* polls, int32_t reset)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    unsigned long long t[kVerdictTally] = {};
    void* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        d = ctx->vtally.p;
    }
    if (d) {   // (never allocated: no stepper began with the option on; zeros, no device call)
        set_device(ctx);
        HCK(hipDeviceSynchronize());
        HCK(hipMemcpy(t, d, sizeof(t), hipMemcpyDeviceToHost));
        if (reset) {   // (complete before the call returns, so before the next launch that adds to it)
            HCK(hipMemsetAsync(d, 0, sizeof(t), nullptr));
            HCK(hipStreamSynchronize(nullptr));
        }
    }
    if (candidates) *candidates = (int64_t)t[0];
    if (rejected_any) *rejected_any = (int64_t)t[1];
    if (rejected_by)
        for (int q = 0; q < kVerdictKinds; ++q) rejected_by[q] = (int64_t)t[2 + q];
    const int64_t np = reset ? ctx->verdict_polls.exchange(0) : ctx->verdict_polls.load();
    if (polls) *polls = np;
    return MAC_OK;
    ABI_END
}

// ---- progressive constraints (k_prog.h; include/maxcover.h mac_prog)

// mac_prog's checks, before the context is touched. *on: a constraint is present.
static int32_t prog_check(const mac_prog* p, int64_t three_n, bool* on)
{
    *on = false;
    if (!p) return MAC_OK;
    if (p->reserved != 0) return fail(MAC_E_INVAL, "mac_prog: reserved must be 0");
    if (p->n_cons < 0 || p->n_cons > kProgMaxJ)
        return fail(MAC_E_INVAL, "mac_prog: n_cons = " + std::to_string(p->n_cons) + " outside [0, " +
                                     std::to_string(kProgMaxJ) + "]");
    if (p->n_cons == 0) return MAC_OK;
    if (!p->member || !p->limit) return fail(MAC_E_INVAL, "mac_prog: n_cons > 0 with a null member or limit array");
    if (three_n < 0) return fail(MAC_E_INVAL, "negative size");
    if (three_n % 3 != 0)
        return fail(MAC_E_SIZE, "InexactError: Int64(" + std::to_string(three_n) + "/3)");
    const int64_t N = three_n / 3;
    if (N > kProgMaxN)
        return fail(MAC_E_INVAL, "mac_prog: N = " + std::to_string(N) + " > " + std::to_string(kProgMaxN) +
                                     " UAVs (the constraint kernel's limit)");
    const uint32_t bad = p->n_cons == 32 ? 0u : ~((1u << p->n_cons) - 1u);
    for (int64_t i = 0; i < N; ++i) {
        if (p->member[i] & bad)
            return fail(MAC_E_INVAL, "mac_prog: member[" + std::to_string(i) + "] has a bit at or above n_cons");
        if (p->limit[i] != p->limit[i])
            return fail(MAC_E_INVAL, "mac_prog: limit[" + std::to_string(i) + "] is NaN");
    }
    *on = true;
    return MAC_OK;
}

// h of one point on the host, the rule's arithmetic (this file is built with contraction off).
static double prog_h_host(const double* x, int N, const mac_prog* p)
{
    double h = 0.0;
    for (int j = 0; j < p->n_cons; ++j) {
        double c = 0.0;
        for (int i = 0; i < N; ++i) {
            if (!((p->member[i] >> j) & 1u)) continue;
            const double d = x[2 * N + i] - p->limit[i];
            c = c + ((d > 0.0 || d != d) ? d : 0.0);
        }
        const double q = c * c;
        h = h + q;
    }
    return h;
}

// member and limit into the lane's buffer: [limit: N doubles][member: N words]
static ProgArgs prog_upload(Lane* L, hipStream_t s, int N, const mac_prog* p)
{
    L->prog.reserve(sizeof(double) * (size_t)N + sizeof(uint32_t) * (size_t)N);
    double* d_limit = L->prog.as<double>();
    uint32_t* d_member = reinterpret_cast<uint32_t*>(d_limit + N);
    // (pageable sources: the copies have left the caller's arrays when they return)
    HCK(hipMemcpyAsync(d_limit, p->limit, sizeof(double) * (size_t)N, hipMemcpyHostToDevice, s));
    HCK(hipMemcpyAsync(d_member, p->member, sizeof(uint32_t) * (size_t)N, hipMemcpyHostToDevice, s));
    return ProgArgs{d_member, d_limit, (int)p->n_cons};
}

int32_t mac_prog_h_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K, const mac_prog* prog,
                       double* h_out)
{
    ABI_BEGIN
    bool on = false;
    int32_t rc = prog_check(prog, three_n, &on);
    if (rc) return rc;
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (three_n < 0 || K < 0) return fail(MAC_E_INVAL, "negative size");
    if (three_n % 3 != 0)
        return fail(MAC_E_SIZE, "InexactError: Int64(" + std::to_string(three_n) + "/3)");
    if (K > (int64_t)1 << 30) return fail(MAC_E_INVAL, "K too large");
    if (K == 0) return MAC_OK;
    if (!h_out) return fail(MAC_E_INVAL, "null h output");
    if (!on || three_n == 0) {   // no constraint, or no UAV to exceed anything
        std::fill(h_out, h_out + K, 0.0);
        return MAC_OK;
    }
    if (!cands) return fail(MAC_E_INVAL, "null candidates");
    const int N = (int)(three_n / 3);
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t in_bytes = sizeof(double) * (size_t)three_n * (size_t)K;
    L->cands.reserve(in_bytes);
    L->progh.reserve(sizeof(double) * (size_t)K);
    HCK(hipMemcpyAsync(L->cands.p, cands, in_bytes, hipMemcpyHostToDevice, s));
    const ProgArgs pa = prog_upload(L, s, N, prog);
    hipLaunchKernelGGL(prog_h_kernel, dim3((unsigned)K), dim3(kProgBlock), 0, s, (uint64_t*)nullptr,
                       matrix_src(L->cands.as<double>(), N), N, pa, (double)INFINITY, L->progh.as<double>(),
                       (uint8_t*)nullptr, 0);
    HCK(hipGetLastError());
    HCK(hipMemcpyAsync(h_out, L->progh.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    return MAC_OK;
    ABI_END
}

// A launch outside the poll chains into mac_profile_kernels' record (role r, nwg workgroups).
static uint64_t* prog_take_ts(mac_ctx* ctx, int role, int64_t nwg)
{
    if (!ctx->profile) return nullptr;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->stamp_used + nwg > ctx->stamp_cap) return nullptr;
    mac_ctx::Prof p{-1, 0, -1, 0, 0, nullptr, ctx->prof.empty() ? 0 : ctx->prof.back().algo};
    p.role[role][0] = ctx->stamp_used;
    p.role[role][1] = nwg;
    uint64_t* ts = ctx->stamps.as<uint64_t>() + 2 * ctx->stamp_used;
    ctx->stamp_used += nwg;
    ctx->prof.push_back(p);
    return ts;
}

constexpr int64_t kProgSelDiagMaxK = 1 << 20;   // mac_diag_prog_select's bound on K

// prog_select_kernel's launch: one workgroup over the (objective, h) arrays of up to two centres, K
// device doubles each (a centre that was not polled: null), the incumbents' scalars by value, the
// record into d_rec. The loop below and mac_diag_prog_select both launch through here.
static void prog_select_launch(hipStream_t s, uint64_t* ts, const double* const obj[2], const double* const h[2],
                               int K, bool has_F, bool has_I, double F_f, double I_f, double I_h, double h_max,
                               ProgRec* d_rec)
{
    ProgSelArgs sa{};
    for (int c = 0; c < 2; ++c) {
        sa.obj[c] = obj[c];
        sa.h[c] = h[c];
    }
    sa.K = K;
    sa.has_F = has_F ? 1 : 0;
    sa.has_I = has_I ? 1 : 0;
    sa.F_f = F_f;
    sa.I_f = I_f;
    sa.I_h = I_h;
    sa.h_max = h_max;
    hipLaunchKernelGGL(prog_select_kernel, dim3(1), dim3(kProgSelBlock), 0, s, ts, sa, d_rec);
    HCK(hipGetLastError());
}

// host only, every build (not declared in maxcover.h): prog_select_kernel on given arrays, through
// the loop's own launch. Centre c: K host doubles of objectives and of h, or both null (the centre
// was not polled); rec8: the 64-byte ProgRec as the kernel wrote it.
int32_t mac_diag_prog_select(mac_ctx* ctx, const double* obj0, const double* h0, const double* obj1,
                             const double* h1, int64_t K, int32_t has_F, int32_t has_I, double F_f, double I_f,
                             double I_h, double h_max, int64_t* rec8)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (!rec8) return fail(MAC_E_INVAL, "null record");
    if (K < 1 || K > kProgSelDiagMaxK)   // (the loop's K is 2 n_p <= 6 kProgMaxN)
        return fail(MAC_E_INVAL, "mac_diag_prog_select: K = " + std::to_string(K) + " outside [1, " +
                                     std::to_string(kProgSelDiagMaxK) + "]");
    if ((obj0 == nullptr) != (h0 == nullptr) || (obj1 == nullptr) != (h1 == nullptr))
        return fail(MAC_E_INVAL, "mac_diag_prog_select: a centre's objectives given without its h, or its h alone");
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t kb = sizeof(double) * (size_t)K;
    L->progobj.reserve(2 * kb);
    L->progh.reserve(2 * kb);
    L->progrec.reserve(sizeof(ProgRec));
    const double* src_obj[2] = {obj0, obj1};
    const double* src_h[2] = {h0, h1};
    const double* d_obj[2] = {nullptr, nullptr};
    const double* d_h[2] = {nullptr, nullptr};
    for (int c = 0; c < 2; ++c) {
        if (!src_obj[c]) continue;
        double* po = L->progobj.as<double>() + (size_t)c * (size_t)K;
        double* ph = L->progh.as<double>() + (size_t)c * (size_t)K;
        HCK(hipMemcpyAsync(po, src_obj[c], kb, hipMemcpyHostToDevice, s));
        HCK(hipMemcpyAsync(ph, src_h[c], kb, hipMemcpyHostToDevice, s));
        d_obj[c] = po;
        d_h[c] = ph;
    }
    prog_select_launch(s, nullptr, d_obj, d_h, (int)K, has_F != 0, has_I != 0, F_f, I_f, I_h, h_max,
                       L->progrec.as<ProgRec>());
    ProgRec r;
    HCK(hipMemcpyAsync(&r, L->progrec.p, sizeof(ProgRec), hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    std::memcpy(rec8, &r, sizeof(ProgRec));
    return MAC_OK;
    ABI_END
}

// prog_part_kernel's launch: one workgroup over a shard's (objective, h) arrays of up to two centres, Kc
// device doubles each (a centre that was not polled: null), the shard's first candidate lo of the poll's
// K, the scalars by value, the 96-byte record into d_part. mac_mads_poll_prog and mac_diag_prog_part both
// launch through here.
static void prog_part_launch(hipStream_t s, uint64_t* ts, const double* const obj[2], const double* const h[2],
                             int Kc, int K, int64_t lo, int64_t tag, const ProgScalars& sc, ProgPart* d_part)
{
    ProgPartArgs pa{};
    for (int c = 0; c < 2; ++c) {
        pa.obj[c] = obj[c];
        pa.h[c] = h[c];
    }
    pa.Kc = Kc;
    pa.K = K;
    pa.lo = lo;
    pa.tag = tag;
    pa.s = sc;
    hipLaunchKernelGGL(prog_part_kernel, dim3(1), dim3(kProgPartBlock), 0, s, ts, pa, d_part);
    HCK(hipGetLastError());
}

// host only, every build (not declared in maxcover.h): prog_part_kernel on given arrays, through the
// stepper's own launch. Centre c: Kc host doubles of objectives and of h (the shard [lo, lo + Kc) of the
// centre's K candidates), or both null; part12: the 96-byte ProgPart as the kernel wrote it.
int32_t mac_diag_prog_part(mac_ctx* ctx, const double* obj0, const double* h0, const double* obj1,
                           const double* h1, int64_t Kc, int64_t K, int64_t lo, int64_t tag, int32_t has_F,
                           int32_t has_I, double F_f, double I_f, double I_h, double h_max, int64_t* part12)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (!part12) return fail(MAC_E_INVAL, "null record");
    if (K < 1 || K > kProgSelDiagMaxK || Kc < 1 || lo < 0 || lo + Kc > K)
        return fail(MAC_E_INVAL, "mac_diag_prog_part: need 1 <= Kc, 0 <= lo, lo + Kc <= K <= " +
                                     std::to_string(kProgSelDiagMaxK));
    if ((obj0 == nullptr) != (h0 == nullptr) || (obj1 == nullptr) != (h1 == nullptr))
        return fail(MAC_E_INVAL, "mac_diag_prog_part: a centre's objectives given without its h, or its h alone");
    set_device(ctx);
    LaneGuard lg(ctx);
    Lane* L = lg.lane;
    hipStream_t s = L->stream;
    const size_t kb = sizeof(double) * (size_t)Kc;
    L->progobj.reserve(2 * kb);
    L->progh.reserve(2 * kb);
    L->progrec.reserve(sizeof(ProgPart));
    const double* src_obj[2] = {obj0, obj1};
    const double* src_h[2] = {h0, h1};
    const double* d_obj[2] = {nullptr, nullptr};
    const double* d_h[2] = {nullptr, nullptr};
    for (int c = 0; c < 2; ++c) {
        if (!src_obj[c]) continue;
        double* po = L->progobj.as<double>() + (size_t)c * (size_t)Kc;
        double* ph = L->progh.as<double>() + (size_t)c * (size_t)Kc;
        HCK(hipMemcpyAsync(po, src_obj[c], kb, hipMemcpyHostToDevice, s));
        HCK(hipMemcpyAsync(ph, src_h[c], kb, hipMemcpyHostToDevice, s));
        d_obj[c] = po;
        d_h[c] = ph;
    }
    const ProgScalars sc{has_F != 0, has_I != 0, F_f, I_f, I_h, h_max};
    prog_part_launch(s, nullptr, d_obj, d_h, (int)Kc, (int)K, lo, tag, sc, L->progrec.as<ProgPart>());
    ProgPart r;
    HCK(hipMemcpyAsync(&r, L->progrec.p, sizeof(ProgPart), hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    std::memcpy(part12, &r, sizeof(ProgPart));
    return MAC_OK;
    ABI_END
}

}  // extern "C" (mads_driver.h opens its own)

// (host only, this file's own: the native MADS driver, on everything above)
#include "mads_driver.h"

extern "C" {

int32_t mac_poll_basis_f64(mac_ctx* ctx, const double* x_inc, int64_t three_n, const int16_t* ltri,
                           const int32_t* rp, const int32_t* cp, double delta, const double* r_max,
                           double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                           double* obj_out, double* best_obj, int64_t* best_idx)
{
    ABI_BEGIN
    return host_eval_basis(ctx, x_inc, three_n, ltri, rp, cp, delta, r_max, penalty, prev, d_lim,
                           tan_half_fov, obj_out, best_obj, best_idx);
    ABI_END
}

int32_t mac_best_reduce_dev(mac_ctx* ctx, const void* d_records, int32_t n_records, void* d_best,
                            void* stream)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (!d_best || (!d_records && n_records > 0)) return fail(MAC_E_INVAL, "null d_best / d_records");
    if (n_records < 0) return fail(MAC_E_INVAL, "negative record count");
    if ((((uintptr_t)d_records) | ((uintptr_t)d_best)) & 7)
        return fail(MAC_E_INVAL, "records / d_best not 8-byte aligned");
    set_device(ctx);
    uint64_t seq = 0;
    uint64_t* d_mirror = assign_mirror(ctx, d_best, &seq);
    hipLaunchKernelGGL(best_reduce_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream,
                       (const unsigned long long*)d_records, (int)n_records, (unsigned long long*)d_best,
                       d_mirror, seq);
    HCK(hipGetLastError());
    return MAC_OK;
    ABI_END
}

// librccl bound once per path (the process keeps it: RCCL is never unloaded under live comms)
static RcclApi* rccl_api(const char* path)
{
    static std::mutex mu;
    static std::vector<std::pair<std::string, RcclApi*>> apis;
    std::lock_guard<std::mutex> lk(mu);
    const std::string key = path ? path : "";
    for (auto& a : apis)
        if (a.first == key) return a.second;
    void* h = nullptr;
    if (path && *path) {
        h = dlopen(path, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);   // the copy already loaded (torch's)
        if (!h) h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    } else {
        h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    if (!h) return nullptr;
    RcclApi* a = new RcclApi();
    a->lib = h;
    a->get_unique_id = (int (*)(RcclUid*))dlsym(h, "ncclGetUniqueId");
    a->comm_init_rank = (int (*)(void**, int, RcclUid, int))dlsym(h, "ncclCommInitRank");
    a->all_gather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))dlsym(h, "ncclAllGather");
    a->comm_destroy = (int (*)(void*))dlsym(h, "ncclCommDestroy");
    a->error_string = (const char* (*)(int))dlsym(h, "ncclGetErrorString");
    if (!a->get_unique_id || !a->comm_init_rank || !a->all_gather || !a->comm_destroy) {
        delete a;
        return nullptr;
    }
    apis.push_back({key, a});
    return a;
}

static int32_t rccl_fail(RcclApi* a, int r, const char* what)
{
    std::string m = std::string(what) + ": RCCL error " + std::to_string(r);
    if (a && a->error_string) m += std::string(" (") + a->error_string(r) + ")";
    return fail(MAC_E_HIP, m.c_str());
}

int32_t mac_comm_unique_id(const char* rccl_path, void* id_out)
{
    ABI_BEGIN
    if (!id_out) return fail(MAC_E_INVAL, "null id");
    RcclApi* a = rccl_api(rccl_path);
    if (!a) return fail(MAC_E_HIP, "cannot load librccl");
    RcclUid id{};
    const int r = a->get_unique_id(&id);
    if (r) return rccl_fail(a, r, "ncclGetUniqueId");
    std::memcpy(id_out, &id, sizeof(id));
    return MAC_OK;
    ABI_END
}

int32_t mac_comm_init(mac_ctx* ctx, const char* rccl_path, const void* id, int32_t rank, int32_t world)
{
    ABI_BEGIN
    if (!ctx || !id) return fail(MAC_E_INVAL, "null context / id");
    if (world < 1 || rank < 0 || rank >= world) return fail(MAC_E_INVAL, "bad rank / world");
    if (ctx->comm) return fail(MAC_E_INVAL, "communicator already set");
    RcclApi* a = rccl_api(rccl_path);
    if (!a) return fail(MAC_E_HIP, "cannot load librccl");
    set_device(ctx);
    RcclUid uid;
    std::memcpy(&uid, id, sizeof(uid));
    void* comm = nullptr;
    const int r = a->comm_init_rank(&comm, world, uid, rank);   // (collective: every rank calls it)
    if (r) return rccl_fail(a, r, "ncclCommInitRank");
    void* buf = nullptr;
    if (hipMalloc(&buf, 16 * (size_t)world) != hipSuccess) {
        (void)a->comm_destroy(comm);
        return fail(MAC_E_NOMEM, "exchange buffer");
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->rccl = a;
    ctx->comm = comm;
    ctx->comm_rank = rank;
    ctx->comm_world = world;
    ctx->d_xrec = buf;
    return MAC_OK;
    ABI_END
}

int32_t mac_exchange_records(mac_ctx* ctx, const void* rec, int32_t bytes, void* out, void* stream)
{
    ABI_BEGIN
    if (!ctx || !rec || !out) return fail(MAC_E_INVAL, "null argument");
    if (!ctx->comm) return fail(MAC_E_INVAL, "no communicator (mac_comm_init)");
    if (bytes <= 0 || bytes > 256 || bytes % 8) return fail(MAC_E_INVAL, "record size: a multiple of 8 up to 256");
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;
    const size_t W = (size_t)ctx->comm_world;
    std::lock_guard<std::mutex> xl(ctx->xmu);   // (one exchange at a time: the buffers are the context's)
    if (!ctx->h_xrec.p) {
        ctx->h_xrec.reserve(256 * (W + 1));
        HCK(hipMalloc(&ctx->d_xrec2, 256 * (W + 1)));
    }
    // this rank's record up, every rank's gathered on the stream, then down: one synchronisation
    unsigned char* h = (unsigned char*)ctx->h_xrec.p;
    unsigned char* d = (unsigned char*)ctx->d_xrec2;
    std::memcpy(h, rec, (size_t)bytes);
    HCK(hipMemcpyAsync(d, h, (size_t)bytes, hipMemcpyHostToDevice, s));
    const int r = ctx->rccl->all_gather(d, d + 256, (size_t)bytes, 1 /* ncclUint8 */, ctx->comm, s);
    if (r) return rccl_fail(ctx->rccl, r, "ncclAllGather");
    HCK(hipMemcpyAsync(h + 256, d + 256, (size_t)bytes * W, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    std::memcpy(out, h + 256, (size_t)bytes * W);
    return MAC_OK;
    ABI_END
}

int32_t mac_poll_exchange(mac_ctx* ctx, const void* d_best, void* d_out, void* stream, double* best_obj,
                          int64_t* best_idx)
{
    ABI_BEGIN
    if (!ctx || !d_best || !d_out) return fail(MAC_E_INVAL, "null argument");
    if (!ctx->comm) return fail(MAC_E_INVAL, "no communicator (mac_comm_init)");
    if ((((uintptr_t)d_best) | ((uintptr_t)d_out)) & 7) return fail(MAC_E_INVAL, "records not 8-byte aligned");
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;
    // every rank's 16-B record into the gather buffer, on the poll's stream (RCCL over xGMI), then
    // one wave's argmin into d_out and its mapped slot, then the slot read (mac_best_fetch)
    const int r = ctx->rccl->all_gather(d_best, ctx->d_xrec, 16, 1 /* ncclUint8 */, ctx->comm, s);
    if (r) return rccl_fail(ctx->rccl, r, "ncclAllGather");
    uint64_t seq = 0;
    uint64_t* d_mirror = assign_mirror(ctx, d_out, &seq);
    hipLaunchKernelGGL(best_reduce_kernel, dim3(1), dim3(kWave), 0, s, (const unsigned long long*)ctx->d_xrec,
                       ctx->comm_world, (unsigned long long*)d_out, d_mirror, seq);
    HCK(hipGetLastError());
    if (!best_obj && !best_idx) return MAC_OK;
    return mac_best_fetch(ctx, d_out, stream, best_obj, best_idx);
    ABI_END
}

int32_t mac_best_fetch(mac_ctx* ctx, const void* d_best, void* stream, double* best_obj,
                       int64_t* best_idx)
{
    ABI_BEGIN
    if (!ctx) return fail(MAC_E_INVAL, "null context");
    if (!d_best) return fail(MAC_E_INVAL, "null d_best");
    set_device(ctx);
    hipStream_t s = (hipStream_t)stream;   // NULL: HIP's null stream
    const uint64_t* slot = nullptr;
    uint64_t want = 0;
    bool pending = false;   // an armed poll on `stream` is not fired: it must not be waited for
    {
        std::lock_guard<std::mutex> lk(ctx->mu);   // (released before any wait)
        for (int q = 0; q < mac_ctx::kMirrorSlots; ++q)
            if (ctx->mirror_key[q] == d_best && ctx->h_mirror.p) {
                slot = (const uint64_t*)ctx->h_mirror.p + 4 * q;
                want = ctx->mirror_want[q];
                break;
            }
        for (auto& a : ctx->armed_on)   // an armed poll on THIS stream is not fired
            pending = pending || (a.first == s && a.second > ctx->fired);
    }
    if (slot) {
        // the latest device poll on d_best writes its result into this slot (the poll takes
        // ~0.1 ms); after 2 ms wait for the stream (which also reports a failed launch), then
        // read the slot once more, else copy d_best
        double o = 0.0;
        int64_t i = -1;
        bool ok = mirror_wait(slot, want, pending ? 2000.0 : 2.0, &o, &i);
        if (!ok && pending)
            return fail(MAC_E_HIP, "poll result not written within 2 s (armed polls pending)");
        if (!ok) {
            HCK(hipStreamSynchronize(s));
            ok = mirror_read(slot, want, &o, &i);
        }
        if (ok) {
            if (best_obj) *best_obj = o;
            if (best_idx) *best_idx = i;
            return MAC_OK;
        }
    }
    double tmp[2];
    HCK(hipMemcpyAsync(tmp, d_best, 16, hipMemcpyDeviceToHost, s));
    HCK(hipStreamSynchronize(s));
    if (best_obj) *best_obj = tmp[0];
    if (best_idx) *best_idx = __builtin_bit_cast(int64_t, tmp[1]);
    return MAC_OK;
    ABI_END
}

}  // extern "C"
