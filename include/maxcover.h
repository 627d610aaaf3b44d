/*
 * maxcover.h — C-ABI of libmaxcover, the MI355X (gfx950) implementation of the
 * MADS area-coverage objective of Gabisanth/MaximumAreaCoverageOptimization.jl.
 *
 * Plain C, no C++ exceptions cross it, no torch types: it is what a Julia
 * `ccall`, a Python `ctypes` stub or any other FFI binds.
 *
 * Reference seam this replaces (paths relative to the reference repo root):
 *   - AreaCoverageCalculation.calculateArea(circles, points)
 *         src/AreaCoverageCalculation.jl:63-110 (live loop :67-78)
 *   - the AreaMaxObjective closure built by TDM_STATIC_opt.createObjective
 *         src/TDM_STATIC_opt.jl:82-100 (penalty :89-97)
 *   - the extreme constraint cons3 built by create_cons3
 *         src/TDM_Constraints.jl:54-75
 *   - CellFunctions.rmvCoveredPOI (order-preserving deletion)
 *         src/CellFunctions.jl:81-108 (predicate :90, deleteat! :101)
 *   - DirectSearch's poll step (evaluate every trial point, keep the best)
 *         called at src/TDM_STATIC_opt.jl:162 (third-party, not vendored)
 *
 * Semantics kept bit-for-bit:
 *   covered(p) = exists c: sqrt((px-cx)^2 + (py-cy)^2) < r_c     (fp64, ^2 = x*x, no FMA,
 *                                                                 correctly rounded sqrt, strict <)
 *   area       = sum of w_p over covered p, w = record column 4   (duplicates counted per entry)
 *   objective  = -area + 1e5 * sum_i |x[2N+i] - r_max[i]|        (sequential sum over i)
 * Candidates use the reference layout [x_1..x_N; y_1..y_N; r_1..r_N] (3N doubles).
 *
 * Ownership: host arrays are borrowed read-only for the duration of a call; the library
 * copies what it keeps into device buffers it owns. Outputs are written before return
 * (synchronous API) except for the *_dev entry points, which are stream-ordered.
 * Threading: mac_area_* / mac_objective_* / mac_poll_* may be called concurrently on one
 * context from several host threads (DirectSearch SetMaxEvals, src/TDM_STATIC_opt.jl:129);
 * mac_set_points_* / mac_remove_covered_* must not overlap evaluations (points only
 * change between MADS calls, src/FullSimulation.jl:50-61).
 */
#ifndef MAXCOVER_H
#define MAXCOVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------------- */
#define MAC_OK            0
#define MAC_E_INVAL       1  /* null pointer / negative size / bad option                    */
#define MAC_E_SIZE        2  /* three_n % 3 != 0: the reference's Int(length/3) InexactError,
                                src/AreaCoverageCalculation.jl:65                            */
#define MAC_E_NOPOINTS    3  /* no point list set on the context                             */
#define MAC_E_HIP         4  /* a HIP runtime call failed (see mac_last_error)               */
#define MAC_E_NOMEM       5  /* device allocation failed                                     */
#define MAC_E_LOSSY       6  /* reserved                                                      */
#define MAC_E_NODEVICE    7  /* no HIP device / bad device index                             */

/* ---- options (mac_set_option) --------------------------------------------------- */
#define MAC_OPT_ALGO         1  /* MAC_ALGO_AUTO (default) | _SCAN | _TILED | _POLL             */
#define MAC_OPT_STORAGE      2  /* MAC_STORE_F64 only: the list is kept in fp64 (fp32 inputs go
                                   through the *_f32 entry points, widened exactly); _F32 fails */
#define MAC_OPT_TILE_POINTS  3  /* target points per spatial tile (default 4), set before points */
#define MAC_OPT_PROFILE      4  /* 1: the timed launches stamp their workgroups' start / end     */
#define MAC_OPT_SHARED       5  /* poll walk, entries two disks' regions share:
                                   MAC_SHARED_AUTO (default) | _FP64 | _BITS                      */

#define MAC_OPT_CHAIN        6  /* the poll chain: MAC_CHAIN_AUTO (default) | _FIVE | _FUSED */

#define MAC_OPT_MESH_KEYS    7  /* how the native MADS driver's polls on a mesh (mac_mads_mesh) key their disks:
                                   MAC_KEYS_VALUE (default) | MAC_KEYS_MESH. Read when a run or a stepper
                                   begins (mac_mads_run_mesh, mac_mads_begin_mesh, mac_mads_run_prog and what is
                                   layered on them); a stepper keeps the mode it began with. Without a mesh
                                   (NULL, or every granularity 1.0) the option changes nothing. Results are
                                   the same under both; only the speed differs.        */

#define MAC_OPT_VERDICTS     8  /* 0 (default) | 1: the native MADS driver tallies what rejected the candidates of
                                   every poll it generates (mac_verdict_read, below). Read when a run or a
                                   stepper begins, as MAC_OPT_MESH_KEYS is; a stepper keeps what it began with.
                                   Results, statistics and the profiled launches are the same under both.       */

#define MAC_KEYS_VALUE   0  /* offsets in metres from candidate 0's disk: exact at any granularity, packed
                               (fast) at integer granularities only                                          */
#define MAC_KEYS_MESH    1  /* the poll's signed integer draws, base the incumbent, scale the disk's
                               granularities: every granularity packs as the unit mesh does                 */

#define MAC_CHAIN_AUTO   0  /* the fused three-launch chain unless one of the context's last 64 polls was crowded,
                               scattered or off the packed-key grid (then the five-launch chain)  */
#define MAC_CHAIN_FIVE   1  /* always the five-launch chain (prep, index, set-up, walk, finalize)   */
#define MAC_CHAIN_FUSED  2  /* the fused chain whenever it applies (K <= 3073, packed keys possible) */

#define MAC_SHARED_AUTO  0  /* bit-word kernel when one of the lane's last 8 polls had more than 16
                               disks with neighbours, else fp64 jobs in the poll kernel         */
#define MAC_SHARED_FP64  1  /* always the poll kernel's fp64 jobs                                */
#define MAC_SHARED_BITS  2  /* always the bit-word kernel (every disk it takes, any count)       */

#define MAC_ALGO_AUTO   0
#define MAC_ALGO_SCAN   1  /* streaming brute-force scan: every point against every disk     */
#define MAC_ALGO_TILED  2  /* per-candidate walk over the tile-binned point list (exact culling) */
#define MAC_ALGO_POLL   3  /* per-disk walk over the whole poll: region entries staged in LDS,
                              one candidate per lane (the six-launch chain; weighted lists) */
/* (4 was an opt-in two-launch poll, measured slower than the chain and removed: refused) */

#define MAC_STORE_F64   0
#define MAC_STORE_F32   1

typedef struct mac_ctx mac_ctx;

/* Thread-local message for the last non-zero status returned on this thread. */
const char* mac_last_error(void);
/* Library version string, e.g. "maxcover 0.1.0 gfx950". */
const char* mac_version(void);

int32_t mac_device_count(int32_t* count_out);
int32_t mac_ctx_create(mac_ctx** out, int32_t device);
void    mac_ctx_destroy(mac_ctx* ctx);
int32_t mac_set_option(mac_ctx* ctx, int32_t option, int64_t value);

/* ---- point list (per MPC step) -------------------------------------------------- */
/* SoA host arrays, M entries each; weight w = the reference's column 4 ("importance"). */
int32_t mac_set_points_f64(mac_ctx* ctx, const double* x, const double* y, const double* w,
                           int64_t M);
/* Reference records: M rows of `stride` doubles, [x, y, area, importance, covered, ...];
 * x = col 1, y = col 2, weight = col 4 (src/AreaCoverageCalculation.jl:16,72). stride >= 4. */
int32_t mac_set_points_records_f64(mac_ctx* ctx, const double* rec, int64_t M, int64_t stride);
/* Same, from device-resident SoA arrays (borrowed for the call, copied). */
int32_t mac_set_points_dev_f64(mac_ctx* ctx, const double* d_x, const double* d_y,
                               const double* d_w, int64_t M);
/* fp32 point lists (SURVEY 8(b) *_f32): each float is widened to the double of the same value
 * on the device and the list is then exactly the fp64 list of those values (the reference's
 * Vector{Float64} would hold the same doubles after Float64(::Float32)). */
int32_t mac_set_points_f32(mac_ctx* ctx, const float* x, const float* y, const float* w,
                           int64_t M);
int32_t mac_set_points_dev_f32(mac_ctx* ctx, const float* d_x, const float* d_y, const float* d_w,
                               int64_t M);
int32_t mac_num_points(mac_ctx* ctx, int64_t* M_out);
/* Copy the current list (original order) back to host SoA arrays (each M_out entries). */
int32_t mac_get_points_f64(mac_ctx* ctx, double* x, double* y, double* w);

/* rmvCoveredPOI (src/CellFunctions.jl:81-108): delete, in place and order-preserving, every
 * entry covered by `circles` ([x;y;r], three_n doubles). kept_idx (nullable, capacity M)
 * receives the 0-based original indices of the kept entries; *M_out the new length. */
int32_t mac_remove_covered_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                               int64_t* kept_idx, int64_t* M_out);
/* Covered flags for the current list (original order), one byte per entry. */
int32_t mac_covered_flags_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                              uint8_t* flags_out);
/* update_POI (src/CellFunctions.jl:59-79): append m entries at the END of the list (list order
 * = summation order), then re-index. Host SoA arrays / device-resident SoA arrays. */
int32_t mac_append_points_f64(mac_ctx* ctx, const double* x, const double* y, const double* w,
                              int64_t m);
int32_t mac_append_points_dev_f64(mac_ctx* ctx, const double* d_x, const double* d_y,
                                  const double* d_w, int64_t m);

/* ---- high-interest regions (src/FullSimulation.jl:751-754) ------------------------ */
/* Axis-aligned boxes the reference's dynamic mode steers the swarm toward. It uses them for the
 * r_max rule (:64-76, host side), for the importance override as a fire point is pushed
 * (src/CellFunctions.jl:42-45 and :68-72) and for the one outcome it prints, "Percentage of Area
 * Covered" (:537-557). The last two run on the device list here (csrc/k_regions.h).
 * Boxes b < n_boxes: (x_lb[b], x_ub[b]) x (y_lb[b], y_ub[b]); membership is the reference's
 *     x < x_ub && x > x_lb && y < y_ub && y > y_lb     (all strict, fp64; NaN anywhere: false),
 * so a box with lb >= ub or a NaN bound holds nothing and an entry with a non-finite coordinate is in
 * no box. w_high: the weight (column 4) given to every INCOMING entry strictly inside any box, the
 * reference's (h_max*tan(FOV/2))^2*pi; NaN: weights are left alone (counting only).
 * n_boxes = 0 (pointers may be NULL): regions off — nothing is launched and every call behaves as
 * if regions did not exist. n_boxes < 0 or > MAC_REGIONS_MAX, or a NULL bound array with
 * n_boxes > 0: MAC_E_INVAL, nothing changed. The call zeroes the ingest counters and touches no
 * weight already in the list.
 * Ingest: while regions are on, the entries arriving through mac_set_points_f64 / _f32 /
 * _records_f64 / _dev_f64 / _dev_f32, mac_append_points_f64 / _dev_f64 and mac_fire_step(append_to)
 * are tested once, in one launch over the incoming range only, after their copy (and widening) into
 * the list and before it is indexed. Entries already in the list are never re-weighted (the reference
 * overrides at push!). mac_set_points_* sets the counters to the new list's counts, an append adds to
 * them, mac_remove_covered_f64 leaves them alone: the union counter is the reference's `total` over
 * every point ever pushed (:539-546).
 * Threading: as mac_set_points_* and mac_covered_flags_f64 — these calls must not overlap an
 * evaluation or a list change. */
#define MAC_REGIONS_MAX 64
int32_t mac_set_regions(mac_ctx* ctx, const double* x_lb, const double* x_ub, const double* y_lb,
                        const double* y_ub, int32_t n_boxes, double w_high);
/* Cumulative counts of the entries that arrived inside the boxes since the counters were last reset:
 * box_count (n_boxes values, nullable) per box, any_count (nullable) for the union, each entry once.
 * Regions off: MAC_E_INVAL. No list is needed (the counters are then zero). */
int32_t mac_regions_ingested(mac_ctx* ctx, int64_t* box_count, int64_t* any_count);
/* The CURRENT list: per box (box_count / box_weight, n_boxes values each) and for the union of the
 * boxes (any_*; an entry counts once, for the lowest-index box holding it) the number of entries
 * and their summed weight; with circles ([x;y;r], three_n doubles; NULL with three_n = 0: none)
 * also the union's entries covered by at least one disk (covered_*; the coverage predicate of
 * mac_area_f64; a disk with r <= 0 or NaN covers nothing; zero without circles). The union's
 * uncovered count after mac_remove_covered_f64 is the reference's `uncovered` (:548-554).
 * Counts are exact. Weight sums are fp64 sums in a fixed order (per-item partials added by a second
 * small launch: the same bits on every run of the same list, options and boxes); when every partial
 * sum is exact they equal the list-order sum bit for bit, otherwise they agree with it to rounding
 * (rtol 1e-12). The kernel reads only the tile rows and columns a box spans, not all M entries.
 * Every output pointer is nullable. Errors (nothing is written): null context, regions off,
 * N > 2048: MAC_E_INVAL; three_n % 3 != 0: MAC_E_SIZE; no list set: MAC_E_NOPOINTS. M = 0: zeros. */
int32_t mac_region_stats_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                             int64_t* box_count, double* box_weight,
                             int64_t* any_count, double* any_weight,
                             int64_t* covered_count, double* covered_weight);

/* ---- objective ------------------------------------------------------------------ */
/* calculateArea(circles, points): one candidate. */
int32_t mac_area_f64(mac_ctx* ctx, const double* circles, int64_t three_n, double* area_out);
/* K candidates, column-major 3N x K (each candidate contiguous, as a Julia Matrix(3N,K)). */
int32_t mac_area_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                           double* area_out);
/* Per-UAV attribution of a candidate's coverage (the credits the reference's first-hit `break`
 * loop sums, src/AreaCoverageCalculation.jl:67-78, kept apart), one kernel launch:
 *   owned[i]     = sum of w_p over entries whose first covering disk in index order is disk i
 *                  (sum_i owned[i] is calculateArea);
 *   exclusive[i] = sum of w_p over entries covered by disk i and by no other disk
 *                  (= area(all disks) - area(all disks but i); exclusive[i] <= owned[i]);
 *   area         = the union's covered weight, the value mac_area_f64 returns.
 * A disk with r <= 0, a NaN radius or a NaN centre covers nothing: it owns nothing and takes
 * nothing from another disk's exclusive part. Of two identical disks the lower index owns their
 * common entries and neither is exclusive there. With equal weights every value is an entry count
 * times the weight (exact; area bit-identical to mac_area_f64); otherwise an fp64 sum in a fixed,
 * run-to-run reproducible order. Every output pointer is nullable, but at least one must be given.
 * N <= 2048 (MAC_E_INVAL above); K = 0 writes nothing; three_n = 0 or an empty list gives zeros.
 * Host calls may run concurrently with mac_area_* / mac_poll_* on one context (not overlapping a
 * point-list change). fp64 callers only: there is no *_f32 form of these calls.
 * One candidate: owned_out / exclusive_out N doubles, area_out one double. */
int32_t mac_area_by_disk_f64(mac_ctx* ctx, const double* circles, int64_t three_n,
                             double* owned_out, double* exclusive_out, double* area_out);
/* K candidates, 3N x K column-major in; owned / exclusive N x K column-major out (candidate k's N
 * values contiguous), area_out K doubles. */
int32_t mac_area_by_disk_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                   double* owned_out, double* exclusive_out, double* area_out);
/* AreaMaxObjective for K candidates: obj_k = -area_k + penalty * sum_i |x[2N+i] - r_max[i]|
 * (penalty = 1e5 in the reference). r_max: N doubles. */
int32_t mac_objective_batch_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                const double* r_max, double penalty, double* obj_out);

/* Poll step: evaluate K candidates, reject those failing cons3 (3-D displacement from
 * `prev` [x;y;r] > d_lim[i], z = R / tan_half_fov; src/TDM_Constraints.jl:54-75) when prev
 * is non-null, and return the lowest-index minimiser (ties -> lowest index, the order a
 * sequential poll keeps its first best). best_idx = -1 when no candidate is feasible.
 * obj_out (nullable, K doubles) receives every objective (+inf for infeasible). As in
 * DirectSearch's extreme barrier, an infeasible candidate is not evaluated: its coverage is never
 * computed (the walks leave it out when N <= 512), only its +inf objective reported. */
int32_t mac_poll_best_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                          const double* r_max, double penalty,
                          const double* prev, const double* d_lim, double tan_half_fov,
                          double* obj_out, double* best_obj, int64_t* best_idx);

/* Basis form of a caller-owned poll (DirectSearch's poll, src/TDM_STATIC_opt.jl:22-44 CustomPoll
 * b / i / maximal_basis; :162): the 2n candidates (n = three_n) x_inc + delta * B[:, k] (index k)
 * and x_inc - delta * B[:, k] (index n + k), k < n, with B = L[rp][:, cp]: B[v][k] =
 * L[rp[v]][cp[k]], L lower triangular, passed as its lower triangle packed by rows (int16, entry
 * (r, c <= r) at r(r+1)/2 + c; n(n+1)/2 entries), rp / cp permutations of [0, n) (any values in
 * [0, n) are accepted). B's entry is delta * L exactly as the double product, so the candidates
 * equal the matrix a caller would build with the same arithmetic, and the results equal
 * mac_poll_best_f64 on that 3N x 2n matrix bit for bit. Ships 16n + n(n+1) bytes instead of 16n^2
 * (config 4: 2.4 MB instead of 37.7 MB). obj_out nullable (2n doubles). */
int32_t mac_poll_basis_f64(mac_ctx* ctx, const double* x_inc, int64_t three_n, const int16_t* ltri,
                           const int32_t* rp, const int32_t* cp, double delta, const double* r_max,
                           double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                           double* obj_out, double* best_obj, int64_t* best_idx);

/* ---- swarm constraints on the device (src/TDM_Constraints.jl cons8, cons7) ---------- */
/* The extreme constraints the reference passes beside cons3 (`cons_ext`, src/FullSimulation.jl:798,
 * handed to MADS as [cons_ext, cons3] at :86 and :97) that concern the swarm as a whole. A candidate
 * is infeasible when any constraint that is on rejects it. A NULL mac_cons* means all off. */
typedef struct mac_cons {
    double d_sep;   /* cons8 (:157-172): infeasible iff some i != j has
                       sqrt((x_i-x_j)^2 + (y_i-y_j)^2) < d_sep (fp64, ^2 = x*x, no FMA, correctly
                       rounded sqrt, strict <; the reference's 15.0). d_sep <= 0 or NaN: off         */
    double zone_y;  /* cons7 (:142-154): infeasible iff some i has y_i < zone_y && r_i > zone_r      */
    double zone_r;  /*        (the reference's 200 and 19*tan(FOV/2)). Either NaN: off                */
} mac_cons;
/* Non-finite inputs follow the reference's arithmetic: a UAV with a NaN or infinite x or y violates
 * the spacing with nobody (sqrt(NaN) < d and inf < d are false) and does not disturb the test of the
 * other UAVs; a NaN y or r never satisfies cons7's comparisons. d_sep = +inf rejects every candidate
 * with two UAVs at a finite squared distance. N = 1 has no pairs: always feasible under cons8.
 * cons4, cons5 and cons6 (:78-138), which limit how a target moves from one MPC step to the next,
 * have a descriptor of their own (mac_motion, below): cons5 is cons3's test with tan_half_fov = 1,
 * but cons3 has one prev / d_lim slot and the reference passes both constraints at once.
 * Caller-owned polls take a mac_cons through the calls below; the native MADS driver (candidates
 * generated on the device) through mac_mads_run_cons / mac_mads_begin_cons.
 *
 * mac_cons_mask: one feasibility byte (1 feasible, 0 infeasible) per candidate of the 3N x K
 * column-major matrix, one kernel launch (k_cons.h: the UAVs counting-sorted by x into cells in LDS,
 * pairs tested up to d_sep apart in x). N <= 2048 (MAC_E_INVAL above, as mac_area_by_disk_*); three_n % 3 != 0: MAC_E_SIZE; K = 0
 * writes nothing. The point list is not read: no list need be set. cons = NULL or all off: every
 * byte 1. The _dev form is stream-ordered and returns after enqueueing. */
int32_t mac_cons_mask_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                          const mac_cons* cons, uint8_t* feasible_out);
int32_t mac_cons_mask_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                              const mac_cons* cons, uint8_t* d_feasible, void* stream);
/* mac_poll_best_f64 under a mac_cons: the result of mac_poll_best_f64 on the same candidates with
 * the objective of every candidate the constraints reject replaced by +inf — the lowest-index
 * minimiser (ties to the lowest original index), {+inf, -1} when nothing is feasible; obj_out holds
 * +inf at rejected candidates and at those failing cons3. Three steps on one stream: the mask
 * launch, the unchanged poll chain, a one-workgroup masked argmin. On this matrix path rejected
 * candidates ARE evaluated by the chain and then discarded (the objective is pure, so the result is
 * the same; the matrix prep kernels take no mask, so that config 4's launches stay as they are). The
 * native MADS driver's generated polls leave them out instead (mac_mads_run_cons). N <= 2048 when a
 * constraint is on. cons = NULL or all off: forwards to mac_poll_best_f64 (bit-identical outputs). Threading as
 * mac_poll_best_f64. */
int32_t mac_poll_best_cons_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                               const double* r_max, double penalty,
                               const double* prev, const double* d_lim, double tan_half_fov,
                               double* obj_out, double* best_obj, int64_t* best_idx,
                               const mac_cons* cons);

/* ---- target-motion constraints on the device (src/TDM_Constraints.jl cons4, cons5, cons6) ---- */
/* The extreme constraints that limit the move of each UAV's target away from the previous MADS
 * target, the anchor a = [x; y; R] (the reference's single_output). For UAV i of a candidate c:
 * t = (c.x_i - a.x_i, c.y_i - a.y_i, c.R_i - a.R_i), q2 = fl(fl(tx*tx) + fl(ty*ty)),
 * q3 = fl(q2 + fl(tz*tz)); fp64 throughout, ^2 = x*x, no FMA, as cons3. A candidate is infeasible
 * iff some i has
 *   cons5 (:106-119)  sqrt(q3) > v_max                        (the reference's 2)
 *   cons6 (:122-138)  |sqrt(q3) - speed_prev[i]| > a_max      (the reference's 1)
 *   cons4 (:78-103)   c < cone_cos,  c = fl(fl(fl(ux*tx) + fl(uy*ty)) /
 *                       fl(fl(sqrt(fl(fl(ux*ux) + fl(uy*uy)))) * fl(sqrt(q2)))),  u = (vx_i, vy_i).
 *                     The reference's abs(acosd(round(c))) > 90 is exactly c < -0.5 (round is
 *                     ties-to-even: round(-0.5) = -0 gives 90 degrees, not > 90), so its value is
 *                     cone_cos = -0.5. A zero velocity or a zero move gives c = NaN: feasible.
 * cons5 and cons6 are decided on q3 against thresholds built on the host (no square root on the
 * device; mac_motion_thresholds); cons4 takes one fp64 square root and one division per UAV.
 * A NaN in any operand follows the arithmetic: every comparison is false and the UAV is feasible.
 * Not pinned: Julia's norm and dot go through a scaled generic_norm2 and BLAS, which may differ from
 * this plain form in the last ulp; parity is pinned against the package's host callables
 * (TDM_Constraints.create_cons4 / 5 / 6), not against Julia. */
typedef struct mac_motion {
    const double* anchor;      /* 3N: the previous target [x; y; R]. NULL: everything off          */
    const double* vel;         /* 2N: [vx; vy], the UAVs' xy velocity (cons4). NULL: cons4 off     */
    const double* speed_prev;  /* N: the norm of the previous target velocity (cons6). NULL: off   */
    double cone_cos;           /* cons4. NaN: off                                                  */
    double v_max;              /* cons5. NaN: off                                                  */
    double a_max;              /* cons6. NaN: off                                                  */
} mac_motion;
/* The three arrays are host pointers, copied at the call (or at mac_mads_begin_motion, for the
 * stepper's lifetime). Each entry point below is the call named in its comment plus a mac_motion;
 * motion = NULL or every constraint off forwards to that call before touching anything (the same
 * launches, bit-identical outputs and statistics). With a constraint on, N <= 2048 (MAC_E_INVAL
 * above), the mask launch also runs with every mac_cons constraint off (without the sort: a load, the
 * tests and one flag per workgroup), and a rejected candidate is treated exactly as a mac_cons
 * rejection is. There are no _dev and no _f32 forms of these calls. */
/* mac_cons_mask_f64 under a mac_motion. */
int32_t mac_cons_mask_motion_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                 const mac_cons* cons, uint8_t* feasible_out, const mac_motion* motion);
/* mac_poll_best_cons_f64 under a mac_motion. */
int32_t mac_poll_best_motion_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                                 const double* r_max, double penalty,
                                 const double* prev, const double* d_lim, double tan_half_fov,
                                 double* obj_out, double* best_obj, int64_t* best_idx,
                                 const mac_cons* cons, const mac_motion* motion);
/* cons6's thresholds for one UAV: |fl(sqrt q3) - speed_prev| > a_max  <=>  q3 > *q_hi || q3 <= *q_lo
 * for every double q3 >= 0 (+inf / -1: that side never rejects). Host arithmetic only; no context. */
void mac_motion_thresholds(double speed_prev, double a_max, double* q_hi, double* q_lo);

/* ---- constraint verdicts: what rejected a candidate ---------------------------------------- */
/* The calls above answer with one feasibility byte, one +inf objective or one count per candidate.
 * A verdict says which constraints reject it, and on which UAVs. Every constraint that is ON is
 * evaluated for every candidate: nothing is short-circuited, neither between constraints nor inside
 * cons8's pair sweep. The defining identity: bit q of `reasons` is set exactly when the existing code
 * rejects the candidate under that constraint alone, i.e. mac_cons_mask_motion_f64 with only that
 * constraint on (kinds 1-5), or the +inf mac_poll_best_f64 reports under prev / d_lim (kind 0). The
 * arithmetic is theirs (fp64, no FMA): cons3's 3-D move against dlim_threshold, cons7's and the
 * motion constraints' per-UAV tests, cons8's pair predicate fl(fl(dx*dx)+fl(dy*dy)) <= T(d_sep) under
 * the same sort and cull (a culled pair is proven feasible, so the pair count is exact). Non-finite
 * inputs behave as in the masks: a UAV with a non-finite x or y is in no pair, a NaN operand rejects
 * nothing. A kind that is OFF has its bit clear, its counts 0 and first_uav = -1; off means
 * prev == NULL (cons3), d_sep <= 0 or NaN (cons8), a NULL descriptor (what it carries), else a NaN
 * scalar or a NULL array exactly as the mask calls decide. All values are integers: they do not
 * depend on thread order. */
#define MAC_VERDICT_KINDS 6
#define MAC_REJ_CONS3 0x01u   /* kind 0: src/TDM_Constraints.jl:54-75  (prev, d_lim)      */
#define MAC_REJ_CONS8 0x02u   /* kind 1: :157-172  spacing    (mac_cons.d_sep)            */
#define MAC_REJ_CONS7 0x04u   /* kind 2: :142-154  zone       (mac_cons.zone_y / zone_r)  */
#define MAC_REJ_CONS4 0x08u   /* kind 3: :78-103   cone       (mac_motion.cone_cos)       */
#define MAC_REJ_CONS5 0x10u   /* kind 4: :106-119  speed      (mac_motion.v_max)          */
#define MAC_REJ_CONS6 0x20u   /* kind 5: :122-138  accel      (mac_motion.a_max)          */
typedef struct mac_verdict {          /* 64 B per candidate */
    uint32_t reasons;                 /* OR of MAC_REJ_* over the constraints that are ON and reject     */
    int32_t  pairs;                   /* cons8: unordered pairs i<j that violate the spacing; 0 when off */
    int32_t  n_uav[MAC_VERDICT_KINDS];     /* per kind: UAVs that violate it (cons8: UAVs in >= 1 such pair) */
    int32_t  first_uav[MAC_VERDICT_KINDS]; /* per kind: the lowest such UAV index, -1 when none            */
    int32_t  reserved[2];             /* written 0 */
} mac_verdict;

/* The verdicts of the K candidates of a 3N x K matrix (column-major, as every batch call takes it),
 * one record each into out. Host pointers, fp64, synchronous; no point list is needed; K = 0 writes
 * nothing. prev / d_lim / tan_half_fov are cons3's inputs as mac_poll_best_f64 takes them. Errors,
 * before anything is launched: a null ctx, or a null out with K > 0: MAC_E_INVAL; three_n % 3 != 0:
 * MAC_E_SIZE; N > 2048: MAC_E_INVAL; prev without d_lim: MAC_E_INVAL. May be called concurrently
 * with evaluations, as mac_cons_mask_f64 may. */
int32_t mac_cons_explain_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K,
                             const double* prev, const double* d_lim, double tan_half_fov,
                             const mac_cons* cons, const mac_motion* motion, mac_verdict* out);

/* The native MADS driver's tally (MAC_OPT_VERDICTS = 1 when the run or stepper began, and cons3, a
 * mac_cons or a mac_motion constraint on): every poll the driver generates (mac_mads_run*'s loop,
 * mac_mads_poll, mac_mads_poll_ahead) enqueues one more launch over its shard, on the poll's stream
 * behind its first launch; it writes scratch of its own and this tally, and nothing of the poll reads
 * it. candidates: candidates examined; rejected_any: those with a non-zero `reasons`;
 * rejected_by[q]: those with bit q set; polls: tallied launches (one per stepper and poll: two
 * steppers that share a poll count it twice). A poll that cons3 rejects whole (rejected_polls) is not
 * launched and not tallied, and neither is a poll the pipelined loop enqueued past its stop; polls
 * ahead are tallied, as feasible_evaluations counts them. Without a mac_prog and with N <= 512,
 * candidates - rejected_any of one stepper's polls is its feasible_evaluations. A run or stepper
 * with a mac_prog ignores the option: the barrier's rejections are visible through mac_prog_h_f64 and
 * mac_mads_prog_stats already (nothing is allocated or checked for it). With the option on and a
 * constraint on (cons3 alone included), a run or stepper over N > 2048 UAVs is MAC_E_INVAL when it
 * begins: the verdict launch sorts in LDS as the mask launch does. The launch stands behind the poll's
 * first (prep) launch, because in the pipelined loop the prep decides the whole-poll rejection. The tally belongs to the context and adds up over its runs and
 * steppers (integer adds: the same totals in any order). The call synchronises the device and
 * copies the tally; every output may be NULL; reset != 0 zeroes it. With the option never set it
 * reports zeros and touches no device. */
int32_t mac_verdict_read(mac_ctx* ctx, int64_t* candidates, int64_t* rejected_any,
                         int64_t* rejected_by /* MAC_VERDICT_KINDS */, int64_t* polls, int32_t reset);

/* ---- native MADS driver ------------------------------------------ */
/* A granular MADS with a complete LTMADS poll, the restatement of DirectSearch's Optimize!
 * (src/TDM_STATIC_opt.jl:118-169; the third-party algorithm is not vendored, so this is the
 * build's own, parity-tested against maximumareacoverageoptimization.jl_amd/TDM_STATIC_opt.mads):
 *   f = objective(x0) (+inf if x0 fails cons3); ell = ell0; per iteration (at most n_iter,
 *   while ell >= 0): B = L[rp][:, cp] with L lower triangular (diagonal +-2^ell, strictly lower
 *   uniform integers in [-(2^ell-1), 2^ell-1]) and random row / column permutations, all drawn
 *   from a splitmix64 stream seeded with `seed`; the 2n candidates x + B[:,k], x - B[:,k] are
 *   generated ON THE DEVICE (no candidate matrix), evaluated with the objective and cons3 as an
 *   extreme barrier; success (best < f): x, f <- best, ell <- min(ell + 1, ell_max); else
 *   ell <- ell - 1. One 16-byte read-back per iteration. */
typedef struct mac_mads_params {
    int64_t n_iter;        /* iteration limit (SetIterationLimit, 100 in the reference)      */
    int32_t ell0, ell_max; /* initial / largest mesh exponent (0 <= ell0 <= ell_max <= 52)    */
    uint64_t seed;
} mac_mads_params;
typedef struct mac_mads_stats {
    double f;              /* objective at x_out (+inf: no feasible point found)              */
    int64_t iterations;
    int64_t evaluations;   /* 1 + 2n per iteration                                            */
    int32_t status;        /* 0: mesh precision limit (ell < 0); 1: iteration limit           */
    int32_t feasible;
    double seconds;        /* wall time inside the call                                       */
    double host_enqueue_s; /* of which: enqueueing the polls (uploads + kernel launches)       */
    double host_perm_s;    /*           next iteration's permutations (overlaps the device)    */
    double wait_s;         /*           waiting for the device                                 */
    double host_post_s;    /*           incumbent update after each poll                       */
    int64_t feasible_evaluations; /* poll candidates that passed cons3 (and the mac_cons, when one is
                                     given) and were evaluated (this stepper's shard; the start
                                     point's evaluation not counted) */
    int64_t rejected_polls;       /* iterations cons3 rejected whole with no evaluation: every
                                     variable's diagonal step +-2^ell alone breaks its UAV's d_lim
                                     (src/TDM_Constraints.jl:67), so no candidate passes — a
                                     failure (ell - 1), as the extreme barrier makes it         */
    int64_t successes;            /* iterations whose poll moved the incumbent (the rest failed) */
    int64_t slot_fallbacks;       /* polls whose result did not arrive through the mapped slot within
                                     50 ms (read by a copy after a stream synchronisation instead):
                                     0 in a healthy run                                           */
} mac_mads_stats;
int32_t mac_mads_run(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                     double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                     const mac_mads_params* params, double* x_out, mac_mads_stats* stats);
/* The same loop under a mac_cons (src/FullSimulation.jl:86,97: MADS gets [cons_ext, cons3]): every
 * poll enqueues one mask launch over its generated candidates before its chain, on the poll's stream
 * (k_cons.h cons_mask_gen_kernel: mac_cons_mask's sort and pair test, one byte per candidate), and
 * the chain's prep launch treats a rejected candidate as a cons3 failure: objective +inf, not
 * evaluated (left out of the walks when N <= 512; evaluated and then +inf above, as cons3 there),
 * not counted in feasible_evaluations. f(x0) is +inf when x0 itself is rejected. cons = NULL or all
 * constraints off: mac_mads_run itself — no mask launch, bit-identical outputs and statistics.
 * N > 2048 with a constraint on: MAC_E_INVAL. */
int32_t mac_mads_run_cons(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                          double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                          const mac_mads_params* params, double* x_out, mac_mads_stats* stats,
                          const mac_cons* cons);

/* The same loop one iteration at a time, for the multi-GPU poll (BASELINE config 5 "8 GPUs";
 * src/TDM_STATIC_opt.jl:129, SetMaxEvals's poll-level parallelism). A stepper owns the shard
 * [shard_lo, shard_hi) of every poll's 2n candidates (0, 2n: the whole poll, as mac_mads_run):
 *   mac_mads_poll    done = 1 once the iteration limit or ell < 0 is reached; otherwise evaluates
 *                    this iteration's shard (generated on the device) and returns its best
 *                    (objective, poll-wide index) (+inf, -1 for an empty shard or no feasible
 *                    candidate);
 *   mac_mads_update  applies the poll's best over ALL shards (the lexicographic (objective,
 *                    index) minimum of the ranks' results, e.g. a 16-B all-gather): the
 *                    incumbent, ell and the stream position advance exactly as in mac_mads_run,
 *                    so every rank stays in lock step with the single-GPU loop;
 *   mac_mads_result  x and the statistics (evaluations count whole polls). */
typedef struct mac_mads mac_mads;
int32_t mac_mads_begin(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                       double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                       const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                       mac_mads** out);
/* mac_mads_begin under a mac_cons (see mac_mads_run_cons): every poll of the stepper — mac_mads_poll
 * and mac_mads_poll_ahead, any shard — is masked; the ranks of a sharded loop pass the same cons. */
int32_t mac_mads_begin_cons(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                            double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                            mac_mads** out, const mac_cons* cons);
int32_t mac_mads_poll(mac_mads* m, int32_t* done, double* best_obj, int64_t* best_idx);
int32_t mac_mads_update(mac_mads* m, double best_obj, int64_t best_idx);
int32_t mac_mads_result(mac_mads* m, double* x_out, mac_mads_stats* stats);
/* Speculation over failure branches (src/TDM_STATIC_opt.jl:162: the MADS iterations are
 * serial, but a failed iteration's next poll is fully determined: the same incumbent, ell - 1, the
 * stream's next position). Rank j of a P-GPU loop evaluates, beside rank 0's real poll, the poll
 * that follows j consecutive failures; after one exchange every rank applies the results in
 * order up to the first success, so a run of failures advances up to P iterations per round:
 *   mac_mads_poll_ahead  evaluates (this stepper's shard of) the poll of the iteration `ahead`
 *                        failures past the current one, without advancing; done = 1 when that
 *                        poll does not exist (iteration limit or ell - ahead < 0); feasible (may be
 *                        NULL): its candidates that passed cons3 and the stepper's mac_cons
 *                        (evaluated);
 *   mac_mads_advance     applies one iteration's result (the poll at ahead = 0) as
 *                        mac_mads_update does, without a prior mac_mads_poll; moved = 1 when the
 *                        incumbent moved (success). Same iterates as the sequential loop. */
int32_t mac_mads_poll_ahead(mac_mads* m, int32_t ahead, int32_t* done, double* best_obj, int64_t* best_idx,
                            int64_t* feasible);
int32_t mac_mads_advance(mac_mads* m, double best_obj, int64_t best_idx, int32_t* moved);
void mac_mads_destroy(mac_mads* m);
/* Every later poll of the stepper also writes its 16-byte shard best {objective, index as
 * int64 bits} to d_best16 (device memory of the context's device, 8-byte aligned; NULL: stop):
 * once mac_mads_poll has returned, the buffer holds that poll's best for device work on any
 * stream (mac_best_fetch's ordering), so a multi-GPU loop all-gathers straight from it with no
 * host-to-device copy per iteration (dist.DeviceGather). */
int32_t mac_mads_best_buffer(mac_mads* m, void* d_best16);

/* The poll kind of the native driver. The reference's CustomPoll "returns directions only in the xy
 * plane. To be used when no height changes need to be explored (i.e. when height constraint is
 * already being satisfied)" (src/TDM_STATIC_opt.jl:15-44, selected at :122): the objective charges
 * 1e5 |R_i - r_max_i| (:92), so once the radii sit at their best granular value every candidate that
 * touches a radius loses, and a full poll's columns are dense below the diagonal. MAC_POLL_XY is that
 * capability on this driver's LTMADS restatement (not the reference's N = 3 ring of 20 directions):
 * with n_p = 2N polled variables x_0..x_{N-1}, y_0..y_{N-1}, every iteration draws the basis
 * B = L[rp][:, cp] of size n_p from the same splitmix64 stream (n_p + n_p(n_p-1)/2 + 2 n_p values
 * per iteration) and polls the 2 n_p = 4N candidates x + E B[:, k] (k < n_p), x - E B[:, k - n_p]
 * (k >= n_p), E putting B's rows on the first 2N variables; a candidate's radii are the incumbent's
 * doubles copied bit for bit, so x_out's radii equal x0's. evaluations grows by 2 n_p per iteration,
 * shards are [lo, hi) within [0, 2 n_p], best_idx is poll-wide in [0, 2 n_p), and the whole-poll
 * rejection (rejected_polls) runs over the n_p polled variables. cons3, the mac_cons mask, the chain
 * routing and the success / failure rule are the full poll's. */
#define MAC_POLL_XYR 0   /* every variable (default) */
#define MAC_POLL_XY  1   /* x and y only: src/TDM_STATIC_opt.jl:15-44 */
typedef struct mac_mads_opts {
    int32_t poll_vars;     /* MAC_POLL_XYR or MAC_POLL_XY */
    int32_t reserved[3];   /* 0 */
} mac_mads_opts;           /* 16 B */
/* mac_mads_run_cons / mac_mads_begin_cons with options (src/TDM_STATIC_opt.jl:118-169, the poll type
 * of :122). opts = NULL or poll_vars = MAC_POLL_XYR: the _cons call itself (cons = NULL: the plain
 * call) — the same launches, outputs and statistics. An unknown poll_vars, a non-zero reserved word
 * or a shard outside [0, 2 n_p]: MAC_E_INVAL, nothing written (*out cleared, as mac_mads_begin_cons
 * does). A stepper begun under MAC_POLL_XY polls xy in every call that takes it (mac_mads_poll,
 * _update, _poll_ahead, _advance, _result, _best_buffer). */
int32_t mac_mads_run_opts(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                          double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                          const mac_mads_params* params, double* x_out, mac_mads_stats* stats,
                          const mac_cons* cons, const mac_mads_opts* opts);
int32_t mac_mads_begin_opts(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                            double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                            mac_mads** out, const mac_cons* cons, const mac_mads_opts* opts);
/* mac_mads_run_opts / mac_mads_begin_opts under a mac_motion (see mac_motion; src/FullSimulation.jl:85,
 * :96 build cons4 in every MPC step): every poll's mask launch also decides the motion constraints, and
 * a rejected candidate is treated as a mac_cons rejection is: not evaluated for N <= 512, evaluated
 * and then +inf above, not counted in feasible_evaluations; f(x0) = +inf when x0 is rejected. Holds
 * under MAC_POLL_XY (the radii stay, so tz = x0's), for any shard and in mac_mads_poll_ahead; the ranks
 * of a sharded loop pass the same motion. motion = NULL or all off: the _opts call itself. */
int32_t mac_mads_run_motion(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                            double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* params, double* x_out, mac_mads_stats* stats,
                            const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion);
int32_t mac_mads_begin_motion(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                              double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                              const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                              mac_mads** out, const mac_cons* cons, const mac_mads_opts* opts,
                              const mac_motion* motion);

/* The mesh of the native driver: DirectSearch's SetGranularity, the one setting the reference's
 * optimize uses (src/TDM_STATIC_opt.jl:131-137; its commented variant keeps 1.0 on the positions and
 * puts 0.1 on the radii). granularity points to 3N host doubles laid out as x (x_0.., y_0.., r_0..),
 * each finite and > 0, copied during the call; NULL is 1.0 everywhere. Polled variable v moves by
 * d = fl(g[v] * (double)L[rp[v]][cp[kk]]), L's entry the integer the stream draws without a mesh (one
 * product), and a candidate's value is x[v] + d (k < n_p) or x[v] - d (k >= n_p): with g[v] = 1.0 the
 * doubles of the calls above bit for bit. The stream, the permutations, the draws per iteration, the
 * success / failure rule, ell_max and the stop at ell < 0 are unchanged; the whole-poll rejection
 * (rejected_polls) tests variable v's diagonal step fl(g[v] * 2^ell). Under MAC_POLL_XY only
 * g[0 .. 2N) is used (the radius entries are still validated). */
typedef struct mac_mads_mesh {
    const double* granularity;   /* 3N host doubles, or NULL (all 1.0) */
    int64_t reserved;            /* 0 */
} mac_mads_mesh;                 /* 16 B */
/* mac_mads_run_motion / mac_mads_begin_motion on a mesh. mesh = NULL, granularity = NULL or every
 * entry exactly 1.0: the _motion call itself — the same launches, outputs and statistics. A zero,
 * negative, NaN or infinite entry or a non-zero reserved word: MAC_E_INVAL (the message names
 * mac_mads_mesh), nothing written and *out cleared, checked before the context is touched. A stepper
 * begun with a mesh uses it in every call that takes it (mac_mads_poll, _update, _poll_ahead,
 * _advance, _result, _best_buffer); the ranks of a sharded loop pass the same vector. */
int32_t mac_mads_run_mesh(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                          double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                          const mac_mads_params* params, double* x_out, mac_mads_stats* stats,
                          const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion,
                          const mac_mads_mesh* mesh);
int32_t mac_mads_begin_mesh(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                            double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                            mac_mads** out, const mac_cons* cons, const mac_mads_opts* opts,
                            const mac_motion* motion, const mac_mads_mesh* mesh);

/* Progressive constraints (src/TDM_Constraints.jl:182-220: cons1_progressive, cons2_progressive,
 * cons3_progressive; handed to DirectSearch's progressive barrier at src/TDM_STATIC_opt.jl:142-159).
 * J = n_cons constraints, 1 <= J <= 32; bit j of member[i] says UAV i belongs to constraint j;
 *   t_i = max(R_i - limit[i], 0.0)   (Julia's max: a NaN difference stays NaN)
 *   c_j = sum of t_i over constraint j's UAVs, folded from 0.0 in the order i = 0 .. N-1
 *   h   = sum_j c_j * c_j, folded from 0.0 in the order j = 0 .. J-1 (each product rounded, no FMA)
 * A point is feasible when h == 0.0 as computed. The arrays are host memory, copied at the call.
 * MAC_E_INVAL (the message names mac_prog, nothing written, checked before the context is touched):
 * n_cons outside [0, 32], n_cons > 0 with a null array, a bit at or above n_cons, a non-zero
 * reserved word, a NaN limit, N > 2048. */
typedef struct mac_prog {
    const uint32_t* member;   /* N host words */
    const double*   limit;    /* N host doubles */
    int32_t         n_cons;   /* 0: no progressive constraint */
    int32_t         reserved; /* = 0 */
    double          h_max0;   /* mac_mads_run_prog: the barrier's first threshold (> 0, +inf allowed);
                                 negative or NaN: h(x0) when that is > 0, else +inf */
} mac_prog;                   /* 32 B */
/* h of the K candidates of a host matrix (3N x K, a candidate per column) into h_out[K], by
 * prog_h_kernel (k_prog.h). Needs no point list. prog = NULL or n_cons = 0: every h is 0.0. */
int32_t mac_prog_h_f64(mac_ctx* ctx, const double* cands, int64_t three_n, int64_t K, const mac_prog* prog,
                       double* h_out);

/* mac_mads_run_mesh under progressive constraints: the progressive barrier (Audet & Dennis 2009) as
 * DESIGN.md section 4 states it. The loop keeps a feasible incumbent F (h == 0) and an infeasible
 * one I (0 < h <= h_max) and polls both with the iteration's one basis (F first); a candidate that
 * fails cons3, mac_cons or mac_motion, whose h is NaN or whose h > h_max is not evaluated. The
 * iteration is dominating (ell + 1), improving (ell stays, h_max drops to the largest candidate h
 * below I.h) or unsuccessful (ell - 1). x_out is F.x when F exists, else I.x
 * (src/TDM_STATIC_opt.jl:165-169); x_inf_out (3N, may be NULL) receives I.x when I exists.
 * stats: f and feasible describe x_out, evaluations = 1 + K per centre polled, successes = the
 * dominating iterations, feasible_evaluations = the candidates evaluated (= pstats->evaluated).
 * The loop is stepped by the host: per iteration and centre the mask launch (if any), prog_h_kernel
 * and the poll chain on one stream, then prog_select_kernel and one read-back of its 64-byte record.
 * prog = NULL or n_cons = 0: mac_mads_run_mesh itself (pstats untouched). Besides mac_prog's errors:
 * h(x0) NaN, h(x0) > h_max0 (MAC_E_INVAL, naming mac_prog, before the context is touched). */
typedef struct mac_mads_prog_stats {
    int32_t has_feasible, has_infeasible;
    double  f_feasible, f_infeasible, h_infeasible, h_max;
    int64_t dominating, improving, unsuccessful;
    int64_t two_centre_polls;
    int64_t evaluated;
} mac_mads_prog_stats;        /* 80 B */
int32_t mac_mads_run_prog(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                          double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                          const mac_mads_params* params, double* x_out, mac_mads_stats* stats,
                          const mac_cons* cons, const mac_mads_opts* opts, const mac_motion* motion,
                          const mac_mads_mesh* mesh, const mac_prog* prog, double* x_inf_out,
                          mac_mads_prog_stats* pstats);

/* The progressive barrier as a stepper: mac_mads_run_prog's loop one iteration at a time over the
 * shard [shard_lo, shard_hi) of every centre's poll, for the sharded and the speculative multi-GPU
 * loops (DESIGN.md section 4 "Progressive barrier": the shard-partial record). A poll reports a
 * mac_prog_part: what steps 3-7 of the rule need from a subset S of the iteration's candidates
 * g = centre K + k (objective +inf: not evaluated; NaN: counted, selects nothing). Every field merges
 * exactly (a sum, an OR, a maximum, or a minimum under a total order with ties to the lower g), so the
 * merged record depends neither on the partition nor on the merge order, and the iterates are
 * mac_mads_run_prog's bit for bit.
 *   tag        the 1-based iteration the record belongs to; bit 62: the loop ends there (done)
 *   evaluated  objectives other than +inf                                                    sum
 *   bestF      min (f, g) over h == 0 (bestF_g < 0: none)                                    min
 *   dominates  an infeasible y with h <= I.h, f <= I.f, one of them strict (with an I only)  OR
 *   h_below    max h over the infeasible y with h < I.h (with an I only; -1.0: none)         max
 *   keep       min (f, h, g) over the infeasible y with h <= I.h (without an I: <= h_max)    min
 *   drop       min (f, h, g) over the infeasible y with h < I.h (with an I only)             min
 * The empty record: (tag, 0, +inf, -1, 0, -1.0, +inf, +inf, -1, +inf, +inf, -1). */
typedef struct mac_prog_part {
    int64_t tag;
    int64_t evaluated;
    double  bestF_f;
    int64_t bestF_g;
    int64_t dominates;
    double  h_below;
    double  keep_f, keep_h;
    int64_t keep_g;
    double  drop_f, drop_h;
    int64_t drop_g;
} mac_prog_part;              /* 96 B */

/* mac_mads_begin_mesh under progressive constraints. prog = NULL or n_cons = 0: mac_mads_begin_mesh
 * itself (a plain stepper). Otherwise mac_mads_run_prog's start: mac_prog's errors, h(x0) NaN and
 * h(x0) > h_max0 (MAC_E_INVAL, naming mac_prog, before the context is touched; *out = NULL); F or I = x0.
 * A prog stepper is stepped by the three calls below alone: mac_mads_poll / _update / _poll_ahead /
 * _advance / _best_buffer return MAC_E_INVAL on it, as the calls below do on a plain stepper.
 * mac_mads_destroy frees either. */
int32_t mac_mads_begin_prog(mac_ctx* ctx, const double* x0, int64_t three_n, const double* r_max,
                            double penalty, const double* prev, const double* d_lim, double tan_half_fov,
                            const mac_mads_params* params, int64_t shard_lo, int64_t shard_hi,
                            mac_mads** out, const mac_cons* cons, const mac_mads_opts* opts,
                            const mac_motion* motion, const mac_mads_mesh* mesh, const mac_prog* prog);
/* The stepper's shard of the polls (F, then I) of the iteration that follows `ahead` iterations which
 * are unsuccessful and leave I as it is (ahead = 0: the current one); the stepper stays as it is.
 * Per centre what mac_mads_run_prog enqueues, over the shard; then prog_part_kernel (k_prog.h, one
 * workgroup, one pass) and one read-back of its 96-byte record. The barrier's threshold: h_max at
 * ahead = 0, else I.h with an I (what an unsuccessful iteration leaves). A centre cons3 rejects whole
 * is not launched; an empty shard launches nothing and reports the empty record. *done = 1 (and bit
 * 62 of the tag) when the loop ends before that iteration. */
int32_t mac_mads_poll_prog(mac_mads* m, int32_t ahead, int32_t* done, mac_prog_part* part);
/* n >= 1 records of one iteration merged into *out (out may be parts). Pure host arithmetic: no
 * context. Unequal tags: MAC_E_INVAL. */
int32_t mac_prog_merge(const mac_prog_part* parts, int32_t n, mac_prog_part* out);
/* Applies the current iteration's merged record (tag = iterations done + 1, else MAC_E_INVAL): steps
 * 3-7 from the record and the stepper's F, I and h_max, the incumbents rebuilt from (centre, k), ell,
 * the counts and the stream advanced. *outcome (may be NULL): 0 dominating, 1 improving, 2
 * unsuccessful. *chains (may be NULL): 1 when the iteration was unsuccessful and left I as it was, so
 * that a record polled one iteration ahead applies next. */
int32_t mac_mads_advance_prog(mac_mads* m, const mac_prog_part* merged, int32_t* outcome, int32_t* chains);
/* mac_mads_run_prog's outputs from a prog stepper: x_out (may be NULL), x_inf_out (may be NULL), stats
 * and pstats with the same meanings; pstats->evaluated sums the applied records' counts, while
 * stats->feasible_evaluations counts what this stepper's own polls evaluated (its shard; polls ahead
 * included). */
int32_t mac_mads_result_prog(mac_mads* m, double* x_out, double* x_inf_out, mac_mads_stats* stats,
                             mac_mads_prog_stats* pstats);

/* fp32 candidates (config 3's "fp32" caller path; SURVEY 8(b) "*_f32: coords f32, accum f64"):
 * the candidate matrix (and prev) are uploaded as floats and widened exactly on the device;
 * coverage is then the reference's fp64 predicate on those doubles, areas accumulate in fp64 /
 * integer counts, and the outputs equal the *_f64 calls on the widened inputs bit for bit.
 * r_max and d_lim stay fp64 (model parameters, not coordinates). */
int32_t mac_area_f32(mac_ctx* ctx, const float* circles, int64_t three_n, double* area_out);
int32_t mac_area_batch_f32(mac_ctx* ctx, const float* cands, int64_t three_n, int64_t K,
                           double* area_out);
int32_t mac_poll_best_f32(mac_ctx* ctx, const float* cands, int64_t three_n, int64_t K,
                          const double* r_max, double penalty, const float* prev,
                          const double* d_lim, double tan_half_fov, double* obj_out,
                          double* best_obj, int64_t* best_idx);

/* ---- device-pointer, stream-ordered variants (inputs already resident in HBM) ----- */
/* d_cands: 3N x K column-major on the context's device; d_area: K doubles. `stream` is a
 * hipStream_t; NULL is HIP's null stream (as in every HIP API: the work is ordered after the
 * caller's default-stream work, e.g. torch's default stream, which produced d_cands). Returns
 * after enqueueing. */
int32_t mac_area_batch_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                               double* d_area, void* stream);
/* mac_area_by_disk_batch_f64 on device pointers, stream-ordered; returns after enqueueing. */
int32_t mac_area_by_disk_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                                 double* d_owned, double* d_exclusive, double* d_area, void* stream);
/* Device poll: d_best receives {best_obj (double), best_idx (int64 stored as double bits)}
 * as 16 bytes; d_obj (nullable) K objectives. d_prev/d_dlim nullable (no cons3). */
int32_t mac_poll_best_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                              const double* d_rmax, double penalty,
                              const double* d_prev, const double* d_dlim, double tan_half_fov,
                              int64_t idx_base, double* d_obj, void* d_best, void* stream);
/* Same with fp32 d_cands / d_prev (widened into the call's scratch on `stream` first). */
int32_t mac_poll_best_dev_f32(mac_ctx* ctx, const float* d_cands, int64_t three_n, int64_t K,
                              const double* d_rmax, double penalty,
                              const float* d_prev, const double* d_dlim, double tan_half_fov,
                              int64_t idx_base, double* d_obj, void* d_best, void* stream);
/* mac_poll_best_dev_f64 under a mac_cons (see mac_poll_best_cons_f64): stream-ordered, no read-back
 * and no synchronisation. The masked argmin writes d_obj, d_best and d_best's mapped slot as the
 * plain poll's finalize does, so mac_best_fetch(d_best) returns the constrained result without a
 * copy. idx_base is added to the index as in the plain call. */
int32_t mac_poll_best_cons_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                                   const double* d_rmax, double penalty,
                                   const double* d_prev, const double* d_dlim, double tan_half_fov,
                                   int64_t idx_base, double* d_obj, void* d_best, void* stream,
                                   const mac_cons* cons);
/* The host side of one MADS poll step: returns the {objective, index} the latest
 * mac_poll_best_dev_* on d_best wrote. Each d_best buffer gets a mapped host slot that the
 * poll's last finalize block fills (after its d_best stores have reached the device's L2), so
 * the call returns as soon as the result exists, without a copy: at that point d_best holds the
 * result for device work, but the poll's launch may still be retiring on `stream` — order later
 * work that reads d_best or reuses the poll's inputs on `stream`, or synchronise it first.
 * Without a slot (a K = 0 poll, or the slot taken by 64 newer d_best buffers) or after 2 ms,
 * it waits for `stream` (NULL: HIP's null stream) and copies d_best. Polls on different
 * d_best buffers may be issued and fetched concurrently from several host threads. */
int32_t mac_best_fetch(mac_ctx* ctx, const void* d_best, void* stream, double* best_obj,
                       int64_t* best_idx);

/* The multi-GPU poll's exchange, reduced on the device: d_records holds n_records 16-B records
 * {objective, index as int64 bits} (the ranks' d_best, e.g. one RCCL all-gather into one buffer
 * ordered on `stream`); one wave writes their lexicographic minimum to d_best (a record with
 * index < 0 or an objective not < +inf never wins; ties to the lowest index; none: {+inf, -1})
 * and to d_best's mapped result slot, so mac_best_fetch(d_best) returns the node's argmin without
 * a copy or a stream synchronisation. Stream-ordered; returns after enqueueing. */
int32_t mac_best_reduce_dev(mac_ctx* ctx, const void* d_records, int32_t n_records, void* d_best,
                            void* stream);

/* The multi-GPU poll exchange over RCCL (xGMI) on the poll's own stream. librccl is bound at run
 * time from rccl_path (the copy the process already loaded when it is loaded, e.g. torch's; NULL:
 * librccl.so.1 from the library path).
 *   mac_comm_unique_id  rank 0 makes the communicator id (128 bytes) the ranks share out of band;
 *   mac_comm_init       every rank (collective) joins with its rank and the world size;
 *   mac_poll_exchange   all-gathers every rank's 16-B {objective, index} record d_best into the
 *                       context's buffer (ncclAllGather on `stream`, ordered after the rank's poll),
 *                       reduces it on the device as mac_best_reduce_dev into d_out and its mapped
 *                       slot, and (best_obj / best_idx non-null) returns the node's argmin from the
 *                       slot as mac_best_fetch does. Collective: every rank calls it per poll.
 * The communicator is destroyed with the context. */
int32_t mac_comm_unique_id(const char* rccl_path, void* id_out);
int32_t mac_comm_init(mac_ctx* ctx, const char* rccl_path, const void* id, int32_t rank, int32_t world);
int32_t mac_poll_exchange(mac_ctx* ctx, const void* d_best, void* d_out, void* stream, double* best_obj,
                          int64_t* best_idx);
/* Every rank's host record of `bytes` bytes (a multiple of 8, at most 256) gathered into `out`
 * (world x bytes, rank order) over the context's communicator: one upload, the all-gather and one
 * download on `stream`, then its synchronisation (the speculative MADS loop's per-round exchange:
 * {done, objective, index, feasible} of every rank's poll). Collective. */
int32_t mac_exchange_records(mac_ctx* ctx, const void* rec, int32_t bytes, void* out, void* stream);

/* Armed device polls: the host turnaround between dependent polls of a MADS loop (the next poll
 * is known only after the previous one's result) taken off the device's critical path. The
 * chain of mac_poll_best_dev_f64 is enqueued ahead of time behind a stream wait on the context's
 * doorbell (a coherent host word the stream waits on), so its launches are already queued
 * when the host decides; mac_poll_fire rings the doorbell and the chain starts without a launch.
 * Its inputs (d_cands, d_prev, ...) may be written until the fire (device writes on other
 * streams must have completed). Rules: tickets are fired in arming order (a fire releases every
 * armed poll with a ticket <= it); a poll and the armed poll after it use different d_best
 * buffers (each buffer's mapped slot follows its latest poll); nothing may wait for the stream
 * (or the device) while an armed poll on it is not fired — mac_best_fetch of a fired poll never
 * does, and mac_ctx_destroy fires every outstanding ticket first. Argument errors are reported
 * before anything is enqueued; a poll that fails after its wait went in voids only its own ticket
 * (released together with the earlier tickets, never ahead of them). `stream` must be a created
 * stream, not NULL (MAC_E_INVAL): an unfired wait on HIP's null stream would block every
 * blocking-stream operation of the process. Buffers an armed poll grows
 * are released at the next device synchronisation (point-list changes, mac_ctx_destroy), since
 * freeing them would wait for the unfired poll. MAC_E_HIP when the device cannot wait on stream
 * values (hipDeviceAttributeCanUseStreamWaitValue). */
int32_t mac_poll_arm_dev_f64(mac_ctx* ctx, const double* d_cands, int64_t three_n, int64_t K,
                             const double* d_rmax, double penalty,
                             const double* d_prev, const double* d_dlim, double tan_half_fov,
                             int64_t idx_base, double* d_obj, void* d_best, void* stream,
                             uint64_t* ticket);
int32_t mac_poll_fire(mac_ctx* ctx, uint64_t ticket);

/* ---- measurement ----------------------------------------------------------------- */
/* With MAC_OPT_PROFILE = 1, the coverage-kernel launches (and the first and last launch of
 * each poll chain) stamp their workgroups' start / end times (s_memrealtime, k_common.h): no
 * packet or dependency is added to the stream. Reads (after a device sync) the summed coverage-
 * kernel time in ms (last end - first start per launch), the launch count and the candidates
 * evaluated by those launches, and the walk the LAST of them used (MAC_ALGO_SCAN / _TILED /
 * _POLL, 0 = none); reset != 0 clears the record. */
int32_t mac_profile_read(mac_ctx* ctx, double* kernel_ms, int64_t* launches,
                         int64_t* candidates, int32_t* last_algo, int32_t reset);

/* Split of the poll chains recorded since the last reset (call before mac_profile_read with
 * reset), summed: launch chain: prep = first launch's first start .. the walk's first start,
 * walk = the walk launch, gap = the walk's last end .. finalize's (+ argmin) last end.
 * polls = chains counted. */
int32_t mac_profile_split(mac_ctx* ctx, double* prep_ms, double* walk_ms, double* gap_ms,
                          int64_t* polls);

/* Per-kernel split of the same poll chains (call before mac_profile_read with reset): for each
 * launch role r < n_roles, the summed launch spans (last workgroup end - first workgroup start,
 * in-kernel stamps) in ms_out[r] and the launches counted in launches_out[r]. Roles:
 *   0 prep_kernel, 1 disk_index_kernel, 2 walk_setup_kernel, 3 coverage_tiled_poll_kernel,
 *   4 coverage_poll_kernel, 5 the crowded-poll shared-entry pass (shared_or_kernel on equal
 *   weights, shared_bits_kernel otherwise), 6 finalize_kernel (five-launch chain), 7 fiw_kernel and
 *   8 fin2_kernel (the fused chain), 9 cons_mask_gen_kernel (the native MADS driver's swarm mask, one
 *   launch per masked poll), 10 prog_h_kernel and 11 prog_select_kernel (mac_mads_run_prog: one
 *   prog_h launch per polled centre, none under MAC_POLL_XY, and one select launch per iteration)
 *   (MAC_PROF_ROLES = 12). */
#define MAC_PROF_ROLES 12
int32_t mac_profile_kernels(mac_ctx* ctx, double* ms_out, int64_t* launches_out, int32_t n_roles);
/* With profiling on, the fused chain's launch-hint reports as the context's later enqueues read them
 * (each poll's finalize writes its report to mapped host words; the lane's next poll reads them, so a
 * report may be read twice or not at all: a sample, not a count of polls): the reports read, and the
 * sum and the largest of hint word 1, the disks of a poll that took one position per candidate (keys
 * that reproduce no double: the identity map). Any output may be NULL; reset != 0 clears the three. */
int32_t mac_profile_fused(mac_ctx* ctx, int64_t* reports, int64_t* ident_sum, int64_t* ident_max, int32_t reset);
/* Host-only diagnostic: what decided the shared entries of the context's most recent poll on the
 * five-launch chain. Synchronises the device, then copies back from that poll's scratch:
 *   words[0]  the walk that ran (1 the poll walk, 2 the per-candidate walk, 0 a stopped loop);
 *   words[1 + q], q < 9: the poll walk's counters: 0 disks with neighbours that qualify for the
 *             bit-word kernel and the union pass, 1 and 3 job counters, 2 disks with neighbours that do
 *             not qualify (an overflowed lower list, or a region past 64 x 64 tiles), 4..7 the union
 *             pass's jobs per weight bucket, 8 disks whose upper list overflowed (the union pass
 *             stands down); words past these are set to 0;
 *   ucount[i], i < n_disks: disk i's distinct positions (the index).
 * Pass that poll's N as n_disks (entries past it are whatever the scratch holds). MAC_E_INVAL when
 * no such poll has run or n_disks exceeds the scratch. Launches nothing. */
int32_t mac_diag_poll_report(mac_ctx* ctx, int32_t* words, int32_t n_words, int32_t* ucount, int32_t n_disks);

/* ---- fire generator (src/DynamicArea.jl, config 5) ------------------------------ */
/* Cellular-automaton forest fire on an nx x ny grid of dx x dy cells, cell (i, j) 1-based with
 * i the row (x index) and j the column (y index), as the reference indexes grid[i, j].
 *   init (:26-35): TREE with probability forest_density else EMPTY; the block
 *                  [ix0, ix1] x [iy0, iy1] (inclusive, 1-based) set to FIRE.
 *   step (:52-72): every interior TREE cell tests each FIRE cell of its 3x3 block, in column-major
 *                  block order, with wind_speed*cos(wind_direction - atan(2-c, 2-r))*prob_spread
 *                  > u; each success makes it FIRE in the new grid and emits one point
 *                  (i*dx - dx/2, j*dy - dy/2, dx*dy, dx*dy, 0) — duplicates per igniting
 *                  neighbour, cells in i-outer/j-inner order (the reference's push order).
 * u is a counter-based hash of (seed, step, cell, neighbour) instead of the reference's unseeded
 * rand(), so runs are reproducible and identical to the CPU restatement. */
typedef struct mac_fire mac_fire;
typedef struct mac_fire_params {
    int64_t nx, ny;                 /* grid size in cells (>= 3 each)                          */
    double dx, dy;                  /* cell pitch (m): 5, 5 in the reference (:6-7)            */
    double forest_density;          /* 0.7 (:20)                                               */
    double prob_spread;             /* 0.5 (:21)                                               */
    double wind_speed;              /* 4 (:47)                                                 */
    double wind_direction;          /* radians; deg2rad(270) (:48)                             */
    int64_t ix0, ix1, iy0, iy1;     /* ignition block, 1-based inclusive (:35)                 */
    uint64_t seed;
} mac_fire_params;
const char* mac_fire_last_error(void);
/* the nine spread thresholds, slot q = (c-1)*3 + (r-1) (column-major block position) */
void    mac_fire_thresholds(const mac_fire_params* p, double* out9);
int32_t mac_fire_create(mac_fire** out, int32_t device, const mac_fire_params* p);
void    mac_fire_destroy(mac_fire* f);
/* :37-42: the initial points (y outer, x inner) as records of 5 doubles; *n_out = count
 * (records written up to cap; rec nullable to query the count). */
int32_t mac_fire_initial_points(mac_fire* f, double* rec, int64_t cap, int64_t* n_out);
/* One update_grid step; *n_new = number of points pushed. They are appended to `append_to`'s
 * list (device to device, update_POI) when non-null. */
int32_t mac_fire_step(mac_fire* f, mac_ctx* append_to, int64_t* n_new);
/* The last step's points as records of 5 doubles (up to cap); *n_out = their count. */
int32_t mac_fire_last_points(mac_fire* f, double* rec, int64_t cap, int64_t* n_out);
/* The current grid, nx*ny bytes, row-major in (i, j): 0 EMPTY, 1 TREE, 2 FIRE. */
int32_t mac_fire_get_grid(mac_fire* f, uint8_t* out);
int32_t mac_fire_set_grid(mac_fire* f, const uint8_t* in);

/* ---- exact predicate helpers (host) --------------------------------------------- */
/* Largest double T with: for every double a >= 0, (sqrt(a) < r) <=> (a <= T), where sqrt is
 * the correctly rounded fp64 sqrt. -1.0 when nothing can be covered (r <= 0 or NaN). */
double mac_cover_threshold(double r);

#ifdef __cplusplus
}
#endif

#endif /* MAXCOVER_H */
