#=
MaxCoverAMD.jl — Julia binding of libmaxcover (include/maxcover.h) for the reference
Gabisanth/MaximumAreaCoverageOptimization.jl. Drop-in replacements for the hot path:

  calculateArea(circles, points)            src/AreaCoverageCalculation.jl:63-110
  createObjective(cells, N, r_max)          src/TDM_STATIC_opt.jl:82-100
  rmvCoveredPOI(cells, circles)             src/CellFunctions.jl:81-108
  poll_best(...)                            DirectSearch's poll step, src/TDM_STATIC_opt.jl:162

Plain `ccall` over the C ABI: no Julia package dependencies. The library path comes from
ENV["MAXCOVER_LIB"] or defaults to the in-tree build. Not executed in this repository's CI
(Julia is not installed in the build image) — the swarm-constraint wrappers (MacCons, cons_mask,
poll_best's `cons`), the verdict wrappers (MacVerdict, cons_explain, set_verdicts!, verdict_read)
and the high-interest region wrappers (set_regions!, regions_ingested, region_stats,
percentage_covered) included; the ctypes mirror
(maximumareacoverageoptimization.jl_amd/_lib.py) makes the same calls with the same arrays and
is what the parity tests exercise. See INTEGRATION.md.
=#
module MaxCoverAMD

export MacContext, set_points!, calculateArea, createObjective, objective_batch, poll_best,
       poll_basis, rmvCoveredPOI!, area_batch, area_by_disk, mads_run, MadsOpts, MacMadsMesh, MacProg, MadsProgStats, MacProgPart, MadsProgStepper,
       mads_prog_stepper, poll_prog!, advance_prog!, prog_merge, result_prog, close_prog!, MacCons, MacMotion, cons_mask,
       set_mesh_keys!, MacVerdict, cons_explain, set_verdicts!, verdict_read,
       set_regions!, clear_regions!, regions_ingested, region_stats, percentage_covered

const libmaxcover = get(ENV, "MAXCOVER_LIB",
    joinpath(@__DIR__, "..", "maximumareacoverageoptimization.jl_amd", "libmaxcover.so"))

const MAC_OK = Int32(0)
const MAC_E_SIZE = Int32(2)

struct MaxCoverError <: Exception
    code::Int32
    msg::String
end
Base.showerror(io::IO, e::MaxCoverError) = print(io, "libmaxcover error ", e.code, ": ", e.msg)

function check(rc::Int32)
    rc == MAC_OK && return nothing
    msg = unsafe_string(ccall((:mac_last_error, libmaxcover), Cstring, ()))
    # the reference's own error for a length that is not a multiple of 3 (Int(length/3))
    rc == MAC_E_SIZE && throw(InexactError(:Int, Int, msg))
    throw(MaxCoverError(rc, msg))
end

"""One device context (one GPU); the point list lives in its HBM between MADS calls."""
mutable struct MacContext
    ptr::Ptr{Cvoid}
    function MacContext(device::Integer = 0)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:mac_ctx_create, libmaxcover), Int32, (Ref{Ptr{Cvoid}}, Int32), out, device))
        ctx = new(out[])
        finalizer(c -> ccall((:mac_ctx_destroy, libmaxcover), Cvoid, (Ptr{Cvoid},), c.ptr), ctx)
        return ctx
    end
end
Base.unsafe_convert(::Type{Ptr{Cvoid}}, c::MacContext) = c.ptr

const _default = Ref{Union{Nothing,MacContext}}(nothing)
default_context() = (_default[] === nothing && (_default[] = MacContext(0)); _default[])

# Vector{Vector{Float64}} records [x, y, area, importance, covered] -> contiguous 5 x M
function pack_records(points::AbstractVector{<:AbstractVector{Float64}})
    M = length(points)
    rec = Matrix{Float64}(undef, 5, M)
    @inbounds for p in 1:M
        r = points[p]
        for j in 1:5
            rec[j, p] = r[j]
        end
    end
    return rec
end

"""Upload the point list (once per MPC step, after the list changes)."""
function set_points!(ctx::MacContext, points::AbstractVector{<:AbstractVector{Float64}})
    rec = pack_records(points)
    check(ccall((:mac_set_points_records_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64), ctx, rec, size(rec, 2), 5))
    return ctx
end

const MAC_OPT_MESH_KEYS = Int32(7)

"""
    set_mesh_keys!(ctx, on)

How `mads_run` polls on a mesh (`MacMadsMesh`) key their disks (MAC_OPT_MESH_KEYS): `false` (default) by
offsets in metres, which pack only at integer granularities; `true` by the poll's signed integer draws,
which pack at every granularity. Results are the same. Read when a run begins.
"""
function set_mesh_keys!(ctx::MacContext, on::Bool)
    check(ccall((:mac_set_option, libmaxcover), Int32, (Ptr{Cvoid}, Int32, Int64), ctx,
                MAC_OPT_MESH_KEYS, on ? 1 : 0))
    return ctx
end

"""calculateArea(circles, points) — src/AreaCoverageCalculation.jl:63-110 (uploads points)."""
function calculateArea(circles::Vector{Float64}, points::AbstractVector{<:AbstractVector{Float64}};
                       ctx::MacContext = default_context())
    set_points!(ctx, points)
    return calculateArea(circles, ctx)
end

"""calculateArea against the context's resident point list."""
function calculateArea(circles::Vector{Float64}, ctx::MacContext)
    out = Ref{Float64}(0.0)
    check(ccall((:mac_area_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Float64}), ctx, circles, length(circles), out))
    return out[]
end

"""
Per-UAV attribution against the context's resident point list: `(owned, exclusive, area)`.
`owned[i]` is the weight of the entries whose first covering disk in index order is disk i
(`sum(owned) == calculateArea`), `exclusive[i]` the weight disk i alone covers.
"""
function area_by_disk(circles::Vector{Float64}, ctx::MacContext)
    length(circles) % 3 == 0 || throw(InexactError(:Int, Int, length(circles) / 3))
    N = div(length(circles), 3)
    owned = zeros(Float64, N)
    exclusive = zeros(Float64, N)
    area = Ref{Float64}(0.0)
    check(ccall((:mac_area_by_disk_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
                ctx, circles, length(circles), owned, exclusive, area))
    return owned, exclusive, area[]
end

"""
High-interest boxes (src/FullSimulation.jl:751-754) on the device list (mac_set_regions). While they
are set, every fire point that arrives in the list (set_points!, the appends, the fire stream)
strictly inside any box — `p[1] .< x_UB .&& p[1] .> x_LB .&& p[2] .< y_UB .&& p[2] .> y_LB`,
src/CellFunctions.jl:42 — gets importance `w_high` (the reference's `(h_max*tan(FOV/2))^2*pi`, :44;
NaN: importances left alone) and is counted. Call it before `set_points!`. At most 64 boxes.
"""
function set_regions!(ctx::MacContext, x_LB::Vector{Float64}, x_UB::Vector{Float64},
                      y_LB::Vector{Float64}, y_UB::Vector{Float64}; w_high::Float64 = NaN)
    n = length(x_LB)
    (length(x_UB) == n && length(y_LB) == n && length(y_UB) == n) ||
        throw(DimensionMismatch("x_LB, x_UB, y_LB, y_UB must have equal lengths"))
    check(ccall((:mac_set_regions, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64),
                ctx, x_LB, x_UB, y_LB, y_UB, n, w_high))
    return ctx
end

clear_regions!(ctx::MacContext) = (check(ccall((:mac_set_regions, libmaxcover), Int32,
    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32, Float64),
    ctx, C_NULL, C_NULL, C_NULL, C_NULL, 0, NaN)); ctx)

"""`(per_box, total)`: the points pushed inside each of the `n_boxes` boxes and inside any of them
(each once) since the list was last set — `total_high_interest_fire_points`, src/FullSimulation.jl:537-546."""
function regions_ingested(ctx::MacContext, n_boxes::Integer)
    per_box = zeros(Int64, max(n_boxes, 1))
    total = Ref{Int64}(0)
    check(ccall((:mac_regions_ingested, libmaxcover), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ref{Int64}),
                ctx, per_box, total))
    return per_box[1:n_boxes], total[]
end

"""
The current list against the boxes (mac_region_stats_f64): per box and for their union (each entry
once) the entry count and summed importance; with `circles` also the union's entries covered by at
least one disk. After `rmvCoveredPOI!`, `any_count` is `uncovered_high_interest_fire_points` (:548-554).
"""
function region_stats(ctx::MacContext, n_boxes::Integer; circles::Vector{Float64} = Float64[])
    bc = zeros(Int64, max(n_boxes, 1))
    bw = zeros(Float64, max(n_boxes, 1))
    ac, cc = Ref{Int64}(0), Ref{Int64}(0)
    aw, cw = Ref{Float64}(0.0), Ref{Float64}(0.0)
    check(ccall((:mac_region_stats_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ref{Int64}, Ref{Float64},
                 Ref{Int64}, Ref{Float64}),
                ctx, isempty(circles) ? C_NULL : pointer(circles), length(circles), bc, bw, ac, aw, cc, cw))
    return (box_count = bc[1:n_boxes], box_weight = bw[1:n_boxes], any_count = ac[], any_weight = aw[],
            covered_count = cc[], covered_weight = cw[])
end

"""src/FullSimulation.jl:557, "Percentage of Area Covered" (0/0 gives NaN, as there)."""
function percentage_covered(ctx::MacContext, n_boxes::Integer)
    total = regions_ingested(ctx, n_boxes)[2]
    uncovered = region_stats(ctx, n_boxes).any_count
    return 100 - (uncovered / total) * 100
end

"""K candidates as the columns of a 3N x K matrix."""
function area_batch(cands::Matrix{Float64}, ctx::MacContext)
    out = Vector{Float64}(undef, size(cands, 2))
    check(ccall((:mac_area_batch_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}),
                ctx, cands, size(cands, 1), size(cands, 2), out))
    return out
end

function objective_batch(cands::Matrix{Float64}, r_max::Vector{Float64}, ctx::MacContext;
                         penalty::Float64 = 1e5)
    out = Vector{Float64}(undef, size(cands, 2))
    check(ccall((:mac_objective_batch_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64, Ptr{Float64}),
                ctx, cands, size(cands, 1), size(cands, 2), r_max, penalty, out))
    return out
end

"""
createObjective(cells, N, r_max) — drop-in for src/TDM_STATIC_opt.jl:82-100.

Uploads `cells.points_of_interest` once (the reference rebuilds the closure every MPC step,
src/FullSimulation.jl:84,95, right after the list changes) and returns the same closure
signature `x::Vector{Float64} -> Float64`: -area + 1e5 * sum |x[2N+i] - r_max[i]|, the penalty
accumulated sequentially on the host exactly as :89-97. `r_max` is captured by reference
(it is mutated between steps, src/FullSimulation.jl:64-76).
"""
function createObjective(cells, N::Integer, r_max::AbstractVector{Float64};
                         ctx::MacContext = default_context())
    set_points!(ctx, cells.points_of_interest)
    function AreaMaxObjective(x::Vector{Float64})
        area = calculateArea(x, ctx)
        violation = 0.0
        for i in 1:N
            violation += abs(x[i + 2N] - r_max[i])
        end
        return -area + violation * 1e5
    end
    return AreaMaxObjective
end

"""
mac_cons (include/maxcover.h): the swarm constraints a poll applies on the GPU, same layout (24 bytes).
`d_sep`: cons8's minimum horizontal spacing (src/TDM_Constraints.jl:157-172; 15.0 there; <= 0 or NaN:
off). `zone_y`, `zone_r`: cons7's altitude zone (:142-154: y < zone_y needs R <= zone_r; 200 and
19*tan(FOV/2) there; either NaN: off). N <= 2048 UAVs.
"""
struct MacCons
    d_sep::Float64
    zone_y::Float64
    zone_r::Float64
end
MacCons(; d_sep::Real = NaN, zone_y::Real = NaN, zone_r::Real = NaN) = MacCons(d_sep, zone_y, zone_r)

"""
MacMotion — the target-motion constraints (mac_motion, include/maxcover.h): cons4 (`cone_cos` with
`vel` = [vx; vy], src/TDM_Constraints.jl:78-103; -0.5 there), cons5 (`v_max`, :106-119; 2) and cons6
(`a_max` with `speed_prev`, :122-138; 1) around the previous target `anchor` = [x; y; R]. A NaN scalar
or `nothing` for its array switches a constraint off. The arrays are copied by each call. Like the
rest of this shim, never executed here.
"""
struct MacMotion
    anchor::Vector{Float64}
    vel::Union{Nothing,Vector{Float64}}
    speed_prev::Union{Nothing,Vector{Float64}}
    cone_cos::Float64
    v_max::Float64
    a_max::Float64
end
MacMotion(anchor::Vector{Float64}; vel = nothing, speed_prev = nothing, cone_cos::Real = NaN,
          v_max::Real = NaN, a_max::Real = NaN) = MacMotion(anchor, vel, speed_prev, cone_cos, v_max, a_max)

# mac_motion's C layout (three host pointers, three doubles); the arrays must be GC.@preserve'd
struct CMotion
    anchor::Ptr{Float64}
    vel::Ptr{Float64}
    speed_prev::Ptr{Float64}
    cone_cos::Float64
    v_max::Float64
    a_max::Float64
end
_ptr_or_null(v) = v === nothing ? Ptr{Float64}(C_NULL) : pointer(v)
CMotion(m::MacMotion) = CMotion(pointer(m.anchor), _ptr_or_null(m.vel), _ptr_or_null(m.speed_prev),
                                m.cone_cos, m.v_max, m.a_max)

"""Feasibility (Bool per column) of the 3N x K candidates under `cons`; needs no point list."""
function cons_mask(cands::Matrix{Float64}, cons::MacCons, ctx::MacContext)
    K = size(cands, 2)
    out = Vector{UInt8}(undef, K)
    check(ccall((:mac_cons_mask_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ref{MacCons}, Ptr{UInt8}),
                ctx, cands, size(cands, 1), K, Ref(cons), out))
    return out .!= 0x00
end

"""
MacVerdict — mac_verdict (include/maxcover.h), the same 64 bytes: what rejected one candidate. `reasons`:
the OR of the kinds' bits (cons3 0x01, cons8 0x02, cons7 0x04, cons4 0x08, cons5 0x10, cons6 0x20) over the
constraints that are on and reject it; `pairs`: cons8's violating unordered pairs; `n_uav[q]` /
`first_uav[q]` (kind q + 1 here: Julia tuples are 1-based; the UAV index itself stays 0-based, -1 = none):
the UAVs whose own test fails and the lowest of them. Written against the header and, like the rest of
this shim, never executed here.
"""
struct MacVerdict
    reasons::UInt32
    pairs::Int32
    n_uav::NTuple{6,Int32}
    first_uav::NTuple{6,Int32}
    reserved::NTuple{2,Int32}
end
const VERDICT_KINDS = (:cons3, :cons8, :cons7, :cons4, :cons5, :cons6)

"""
cons_explain(cands, ctx; cons, motion, prev, d_lim, tan_half_fov) — mac_cons_explain_f64: one MacVerdict
per column of the 3N x K candidates. Every constraint that is on is evaluated for every candidate (no
short-circuit); cons3 through `prev` / `d_lim` as poll_best takes them. Needs no point list.
"""
function cons_explain(cands::Matrix{Float64}, ctx::MacContext; cons::Union{Nothing,MacCons} = nothing,
                      motion::Union{Nothing,MacMotion} = nothing,
                      prev::Union{Nothing,Vector{Float64}} = nothing,
                      d_lim::Union{Nothing,Vector{Float64}} = nothing, tan_half_fov::Float64 = 1.0)
    K = size(cands, 2)
    out = Vector{MacVerdict}(undef, K)
    rcons = cons === nothing ? nothing : Ref(cons)
    rmot = motion === nothing ? nothing : Ref(CMotion(motion))
    GC.@preserve prev d_lim motion rcons rmot begin
        check(ccall((:mac_cons_explain_f64, libmaxcover), Int32,
                    (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64,
                     Ptr{MacCons}, Ptr{CMotion}, Ptr{MacVerdict}),
                    ctx, cands, size(cands, 1), K, _ptr_or_null(prev), _ptr_or_null(d_lim), tan_half_fov,
                    rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons),
                    rmot === nothing ? Ptr{CMotion}(C_NULL) : Base.unsafe_convert(Ptr{CMotion}, rmot), out))
    end
    return out
end

const MAC_OPT_VERDICTS = Int32(8)

"""
    set_verdicts!(ctx, on)

Whether `mads_run` tallies what rejected the candidates of the polls it generates (MAC_OPT_VERDICTS;
`verdict_read`). Read when a run begins; results are the same either way; a run with a `MacProg` ignores it.
"""
function set_verdicts!(ctx::MacContext, on::Bool)
    check(ccall((:mac_set_option, libmaxcover), Int32, (Ptr{Cvoid}, Int32, Int64), ctx,
                MAC_OPT_VERDICTS, on ? 1 : 0))
    return ctx
end

"""
verdict_read(ctx; reset = true) — mac_verdict_read: (candidates, rejected_any, rejected_by, polls) since
the last reset, `rejected_by` a NamedTuple over VERDICT_KINDS. Synchronises the device.
"""
function verdict_read(ctx::MacContext; reset::Bool = true)
    c, a, p = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
    by = zeros(Int64, 6)
    check(ccall((:mac_verdict_read, libmaxcover), Int32,
                (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ref{Int64}, Int32),
                ctx, c, a, by, p, reset ? 1 : 0))
    return (candidates = c[], rejected_any = a[], rejected_by = NamedTuple{VERDICT_KINDS}(Tuple(by)),
            polls = p[])
end

"""
poll_best(cands, r_max; prev, d_lim, tan_half_fov, cons) — one whole MADS poll on the GPU: every
candidate's objective, cons3 (src/TDM_Constraints.jl:54-75) as an extreme barrier (+Inf), and
the lowest-index minimiser. With `cons::MacCons` (mac_poll_best_cons_f64) the candidates cons8 /
cons7 reject are +Inf as well (on this matrix path they are still evaluated by the chain, then
discarded; mads_run's generated polls leave them out); `nothing`
keeps the plain call. Returns (best_obj, best_idx (1-based, 0 if none feasible), objs).
"""
function poll_best(cands::Matrix{Float64}, r_max::Vector{Float64}, ctx::MacContext;
                   penalty::Float64 = 1e5, prev::Union{Nothing,Vector{Float64}} = nothing,
                   d_lim::Union{Nothing,Vector{Float64}} = nothing, tan_half_fov::Float64 = 1.0,
                   cons::Union{Nothing,MacCons} = nothing, motion::Union{Nothing,MacMotion} = nothing)
    K = size(cands, 2)
    objs = Vector{Float64}(undef, K)
    bo = Ref{Float64}(Inf)
    bi = Ref{Int64}(-1)
    pprev = prev === nothing ? Ptr{Float64}(C_NULL) : pointer(prev)
    pdlim = d_lim === nothing ? Ptr{Float64}(C_NULL) : pointer(d_lim)
    GC.@preserve prev d_lim motion begin
        if motion !== nothing   # mac_poll_best_motion_f64: cons4 / cons5 / cons6 as well
            rcons = cons === nothing ? nothing : Ref(cons)
            GC.@preserve rcons begin
                pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
                check(ccall((:mac_poll_best_motion_f64, libmaxcover), Int32,
                            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64,
                             Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{Float64}, Ref{Int64},
                             Ptr{MacCons}, Ref{CMotion}),
                            ctx, cands, size(cands, 1), K, r_max, penalty, pprev, pdlim, tan_half_fov,
                            objs, bo, bi, pcons, Ref(CMotion(motion))))
            end
        elseif cons === nothing
            check(ccall((:mac_poll_best_f64, libmaxcover), Int32,
                        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64,
                         Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{Float64}, Ref{Int64}),
                        ctx, cands, size(cands, 1), K, r_max, penalty, pprev, pdlim, tan_half_fov,
                        objs, bo, bi))
        else
            check(ccall((:mac_poll_best_cons_f64, libmaxcover), Int32,
                        (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64,
                         Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Ref{Float64}, Ref{Int64},
                         Ref{MacCons}),
                        ctx, cands, size(cands, 1), K, r_max, penalty, pprev, pdlim, tan_half_fov,
                        objs, bo, bi, Ref(cons)))
        end
    end
    return bo[], bi[] + 1, objs
end

"""
The device-pointer forms (mac_cons_mask_dev_f64, mac_poll_best_cons_dev_f64: stream-ordered, no
read-back) for callers that keep the candidates in HBM (AMDGPU.jl arrays): raw pointers and a
hipStream_t, as mac_poll_best_dev_f64.
"""
function cons_mask_dev(d_cands::Ptr{Float64}, three_n::Integer, K::Integer, cons::MacCons,
                       d_feasible::Ptr{UInt8}, ctx::MacContext; stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:mac_cons_mask_dev_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ref{MacCons}, Ptr{UInt8}, Ptr{Cvoid}),
                ctx, d_cands, three_n, K, Ref(cons), d_feasible, stream))
end

function poll_best_cons_dev(d_cands::Ptr{Float64}, three_n::Integer, K::Integer, d_rmax::Ptr{Float64},
                            d_best::Ptr{Cvoid}, cons::MacCons, ctx::MacContext; penalty::Float64 = 1e5,
                            d_prev::Ptr{Float64} = Ptr{Float64}(C_NULL),
                            d_dlim::Ptr{Float64} = Ptr{Float64}(C_NULL), tan_half_fov::Float64 = 1.0,
                            idx_base::Integer = 0, d_obj::Ptr{Float64} = Ptr{Float64}(C_NULL),
                            stream::Ptr{Cvoid} = C_NULL)
    check(ccall((:mac_poll_best_cons_dev_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                 Ptr{Float64}, Float64, Int64, Ptr{Float64}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{MacCons}),
                ctx, d_cands, three_n, K, d_rmax, penalty, d_prev, d_dlim, tan_half_fov, idx_base,
                d_obj, d_best, stream, Ref(cons)))
end

"""
poll_basis(x_inc, L, rp, cp, delta, r_max, ctx; prev, d_lim, tan_half_fov) — a DirectSearch-owned
poll in basis form (src/TDM_STATIC_opt.jl:22-44 CustomPoll's b / i / maximal_basis; :162): the 2n
candidates x_inc ± delta * B[:, k], B = L[rp, cp] (L lower triangular, rp / cp permutations,
1-based here as in Julia), expanded on the GPU — 2.4 MB shipped at n = 1536 instead of the 37.7-MB
matrix. Returns (best_obj, best_idx (1-based over [plus directions; minus directions], 0 if none
feasible), objs).
"""
function poll_basis(x_inc::Vector{Float64}, L::AbstractMatrix{<:Integer}, rp::AbstractVector{<:Integer},
                    cp::AbstractVector{<:Integer}, delta::Float64, r_max::Vector{Float64},
                    ctx::MacContext; penalty::Float64 = 1e5,
                    prev::Union{Nothing,Vector{Float64}} = nothing,
                    d_lim::Union{Nothing,Vector{Float64}} = nothing, tan_half_fov::Float64 = 1.0)
    n = length(x_inc)
    tri = Vector{Int16}(undef, n * (n + 1) ÷ 2)
    q = 1
    @inbounds for r in 1:n, c in 1:r      # lower triangle packed by rows
        tri[q] = Int16(L[r, c])
        q += 1
    end
    rp0 = Int32.(rp .- 1)
    cp0 = Int32.(cp .- 1)
    objs = Vector{Float64}(undef, 2n)
    bo = Ref{Float64}(Inf)
    bi = Ref{Int64}(-1)
    pprev = prev === nothing ? Ptr{Float64}(C_NULL) : pointer(prev)
    pdlim = d_lim === nothing ? Ptr{Float64}(C_NULL) : pointer(d_lim)
    GC.@preserve prev d_lim begin
        check(ccall((:mac_poll_basis_f64, libmaxcover), Int32,
                    (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int16}, Ptr{Int32}, Ptr{Int32}, Float64,
                     Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64},
                     Ref{Float64}, Ref{Int64}),
                    ctx, x_inc, n, tri, rp0, cp0, delta, r_max, penalty, pprev, pdlim, tan_half_fov,
                    objs, bo, bi))
    end
    return bo[], bi[] + 1, objs
end

struct MadsParams
    n_iter::Int64
    ell0::Int32
    ell_max::Int32
    seed::UInt64
end
struct MadsStats
    f::Float64
    iterations::Int64
    evaluations::Int64
    status::Int32
    feasible::Int32
    seconds::Float64
    host_enqueue_s::Float64
    host_perm_s::Float64
    wait_s::Float64
    host_post_s::Float64
    feasible_evaluations::Int64
    rejected_polls::Int64
    successes::Int64
    slot_fallbacks::Int64
end

"""
MadsOpts — mac_mads_opts (include/maxcover.h), 16 bytes: the native driver's poll kind, MAC_POLL_XYR
(0: every variable) or MAC_POLL_XY (1: x and y only, the radii held; the reference's CustomPoll,
src/TDM_STATIC_opt.jl:15-44); the reserved words are 0.
"""
struct MadsOpts
    poll_vars::Int32
    reserved1::Int32
    reserved2::Int32
    reserved3::Int32
end
MadsOpts(poll_vars::Symbol) = MadsOpts(poll_vars === :xyr ? Int32(0) : poll_vars === :xy ? Int32(1) :
                                       throw(ArgumentError("poll_vars must be :xyr or :xy")),
                                       Int32(0), Int32(0), Int32(0))

"""
MacMadsMesh — mac_mads_mesh (include/maxcover.h), 16 bytes: the native driver's per-variable granularity
(DirectSearch's SetGranularity, src/TDM_STATIC_opt.jl:131-137): a pointer to 3N host doubles laid out as
x (C_NULL: 1.0 everywhere), copied during the call, and a reserved word that is 0.
"""
struct MacMadsMesh
    granularity::Ptr{Float64}
    reserved::Int64
end

"The 3N granularities of `granularity`: a number, a pair (g_xy, g_r) or 3N numbers, each finite and > 0."
function mesh_granularity(granularity, three_n::Integer)
    N = three_n ÷ 3
    g = granularity isa Real ? fill(Float64(granularity), three_n) :
        length(granularity) == 2 ? vcat(fill(Float64(granularity[1]), 2N), fill(Float64(granularity[2]), three_n - 2N)) :
        length(granularity) == three_n ? Vector{Float64}(collect(granularity)) :
        throw(ArgumentError("granularity must be a number, a pair (g_xy, g_r) or $three_n numbers"))
    all(v -> isfinite(v) && v > 0, g) || throw(ArgumentError("granularity: every entry must be finite and > 0"))
    return g
end

"""
MacProg — the progressive constraints of src/TDM_Constraints.jl:182-220 (mac_prog, include/maxcover.h):
bit j of `member[i]` says UAV i belongs to constraint j (1 <= n_cons <= 32), `limit[i]` is its altitude
limit (r_max), `h_max0` the progressive barrier's first threshold (negative: h(x0), the reference's
barrier_threshold^2, src/TDM_STATIC_opt.jl:146). `MacProg(r_max)` is cons1_progressive: every UAV in
one constraint.
"""
struct MacProg
    member::Vector{UInt32}
    limit::Vector{Float64}
    n_cons::Int32
    h_max0::Float64
end
MacProg(r_max::Vector{Float64}; h_max0::Float64 = -1.0) =
    MacProg(fill(UInt32(1), length(r_max)), copy(r_max), Int32(1), h_max0)

struct CProg   # mac_prog's C layout, 32 bytes
    member::Ptr{UInt32}
    limit::Ptr{Float64}
    n_cons::Int32
    reserved::Int32
    h_max0::Float64
end

"mac_mads_prog_stats (include/maxcover.h), 80 bytes."
struct MadsProgStats
    has_feasible::Int32
    has_infeasible::Int32
    f_feasible::Float64
    f_infeasible::Float64
    h_infeasible::Float64
    h_max::Float64
    dominating::Int64
    improving::Int64
    unsuccessful::Int64
    two_centre_polls::Int64
    evaluated::Int64
end

"""
mads_run(x0, r_max, ctx; prev, d_lim, tan_half_fov, n_iter, ell0, ell_max, seed, cons, poll_vars) — the whole
granular-MADS loop inside libmaxcover (complete LTMADS poll generated on the device, cons3 as
extreme barrier): the batched stand-in for TDM_STATIC_opt.optimize (src/TDM_STATIC_opt.jl:118-169).
With `cons::MacCons` (mac_mads_run_cons) every poll also applies cons8 / cons7 on the device — the
`cons_ext` slot of the reference's [cons_ext, cons3] — and the candidates they reject are not
evaluated; `nothing` keeps the plain call. `poll_vars = :xy` (mac_mads_run_opts, MAC_POLL_XY) polls
x and y only — 4N candidates per poll from a basis of size 2N, the radii of `x` equal to `x0`'s bit
for bit — for the steps where "no height changes need to be explored" (src/TDM_STATIC_opt.jl:15-44);
`:xyr`, the default, is the calls above. `motion::MacMotion` (mac_mads_run_motion) adds cons4 / cons5 /
cons6 to every poll's mask. `granularity` (mac_mads_run_mesh; `nothing`: the calls above): a number, a pair
(g_xy, g_r) or 3N numbers laid out as `x0`; variable v then steps by g[v] times the basis's integers, as the
reference's SetGranularity does (:131-137). `prog::MacProg` (mac_mads_run_prog): the reference's
`cons_prog` slot under the progressive barrier; the call then returns
(x, stats::MadsStats, x_infeasible, pstats::MadsProgStats), x the feasible incumbent when there is one
(src/TDM_STATIC_opt.jl:165-169) and x_infeasible the infeasible one or `nothing`. Like the rest of this
shim, the `poll_vars`, `motion`, `granularity` and `prog` paths have not been executed here. Returns
(x, stats::MadsStats).
"""
function mads_run(x0::Vector{Float64}, r_max::Vector{Float64}, ctx::MacContext;
                  penalty::Float64 = 1e5, prev::Union{Nothing,Vector{Float64}} = nothing,
                  d_lim::Union{Nothing,Vector{Float64}} = nothing, tan_half_fov::Float64 = 1.0,
                  n_iter::Integer = 100, ell0::Integer = 2, ell_max::Integer = 6,
                  seed::Integer = 20250216, cons::Union{Nothing,MacCons} = nothing,
                  poll_vars::Symbol = :xyr, motion::Union{Nothing,MacMotion} = nothing,
                  granularity = nothing, prog::Union{Nothing,MacProg} = nothing)
    opts = MadsOpts(poll_vars)
    g = granularity === nothing ? nothing : mesh_granularity(granularity, length(x0))
    x = similar(x0)
    prm = Ref(MadsParams(n_iter, ell0, ell_max, UInt64(seed)))
    st = Ref{MadsStats}()
    pprev = prev === nothing ? Ptr{Float64}(C_NULL) : pointer(prev)
    pdlim = d_lim === nothing ? Ptr{Float64}(C_NULL) : pointer(d_lim)
    if prog !== nothing
        length(prog.member) == length(prog.limit) == length(x0) ÷ 3 ||
            throw(ArgumentError("prog: member and limit hold N values each"))
        xi = fill(NaN, length(x0))
        ps = Ref{MadsProgStats}()
        rcons = cons === nothing ? nothing : Ref(cons)
        rmot = motion === nothing ? nothing : Ref(CMotion(motion))
        rmesh = g === nothing ? nothing : Ref(MacMadsMesh(pointer(g), 0))
        GC.@preserve prev d_lim motion g prog rcons rmot rmesh begin
            pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
            pmot = rmot === nothing ? Ptr{CMotion}(C_NULL) : Base.unsafe_convert(Ptr{CMotion}, rmot)
            pmesh = rmesh === nothing ? Ptr{MacMadsMesh}(C_NULL) : Base.unsafe_convert(Ptr{MacMadsMesh}, rmesh)
            cp = Ref(CProg(pointer(prog.member), pointer(prog.limit), prog.n_cons, Int32(0), prog.h_max0))
            check(ccall((:mac_mads_run_prog, libmaxcover), Int32,
                        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                         Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats},
                         Ptr{MacCons}, Ref{MadsOpts}, Ptr{CMotion}, Ptr{MacMadsMesh}, Ref{CProg},
                         Ptr{Float64}, Ref{MadsProgStats}),
                        ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st,
                        pcons, Ref(opts), pmot, pmesh, cp, xi, ps))
        end
        return x, st[], (ps[].has_infeasible != 0 ? xi : nothing), ps[]
    end
    GC.@preserve prev d_lim motion g begin
        if g !== nothing
            rcons = cons === nothing ? nothing : Ref(cons)
            rmot = motion === nothing ? nothing : Ref(CMotion(motion))
            GC.@preserve rcons rmot begin
                pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
                pmot = rmot === nothing ? Ptr{CMotion}(C_NULL) : Base.unsafe_convert(Ptr{CMotion}, rmot)
                check(ccall((:mac_mads_run_mesh, libmaxcover), Int32,
                            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                             Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats},
                             Ptr{MacCons}, Ref{MadsOpts}, Ptr{CMotion}, Ref{MacMadsMesh}),
                            ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st,
                            pcons, Ref(opts), pmot, Ref(MacMadsMesh(pointer(g), 0))))
            end
        elseif motion !== nothing
            rcons = cons === nothing ? nothing : Ref(cons)
            GC.@preserve rcons begin
                pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
                check(ccall((:mac_mads_run_motion, libmaxcover), Int32,
                            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                             Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats},
                             Ptr{MacCons}, Ref{MadsOpts}, Ref{CMotion}),
                            ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st,
                            pcons, Ref(opts), Ref(CMotion(motion))))
            end
        elseif opts.poll_vars != 0
            rcons = cons === nothing ? nothing : Ref(cons)   # (kept alive across the call)
            GC.@preserve rcons begin
                pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
                check(ccall((:mac_mads_run_opts, libmaxcover), Int32,
                            (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                             Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats},
                             Ptr{MacCons}, Ref{MadsOpts}),
                            ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st,
                            pcons, Ref(opts)))
            end
        elseif cons === nothing
            check(ccall((:mac_mads_run, libmaxcover), Int32,
                        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                         Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats}),
                        ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st))
        else
            check(ccall((:mac_mads_run_cons, libmaxcover), Int32,
                        (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64},
                         Ptr{Float64}, Float64, Ref{MadsParams}, Ptr{Float64}, Ref{MadsStats},
                         Ref{MacCons}),
                        ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, x, st,
                        Ref(cons)))
        end
    end
    return x, st[]
end

"""
MacProgPart — mac_prog_part (include/maxcover.h), 96 bytes: the shard-partial record of one iteration of
the progressive barrier, what a rank's poll reports and what the ranks exchange and merge. `tag`: the
1-based iteration, bit 62 set when the loop ends there.
"""
struct MacProgPart
    tag::Int64
    evaluated::Int64
    bestF_f::Float64
    bestF_g::Int64
    dominates::Int64
    h_below::Float64
    keep_f::Float64
    keep_h::Float64
    keep_g::Int64
    drop_f::Float64
    drop_h::Float64
    drop_g::Int64
end

"A prog stepper's handle (mac_mads*) with its context and size; `close_prog!` frees it."
mutable struct MadsProgStepper
    handle::Ptr{Cvoid}
    ctx::MacContext
    n::Int
end

"""
mads_prog_stepper(x0, r_max, ctx; prog, shard = nothing, ...) — mac_mads_begin_prog: `mads_run(...; prog)`'s
loop one iteration at a time over the candidate shard `shard = (lo, hi)` (0-based, half-open; nothing: the
whole poll) of every centre's poll. Drive it with `poll_prog!`, `prog_merge` over the ranks' records and
`advance_prog!`. The keywords are `mads_run`'s; every rank passes the same ones. Like the rest of the shim
these wrappers have not been executed here.
"""
function mads_prog_stepper(x0::Vector{Float64}, r_max::Vector{Float64}, ctx::MacContext; prog::MacProg,
                           shard = nothing, penalty::Float64 = 1e5,
                           prev::Union{Nothing,Vector{Float64}} = nothing,
                           d_lim::Union{Nothing,Vector{Float64}} = nothing, tan_half_fov::Float64 = 1.0,
                           n_iter::Integer = 100, ell0::Integer = 2, ell_max::Integer = 6,
                           seed::Integer = 20250216, cons::Union{Nothing,MacCons} = nothing,
                           poll_vars::Symbol = :xyr, motion::Union{Nothing,MacMotion} = nothing,
                           granularity = nothing)
    length(prog.member) == length(prog.limit) == length(x0) ÷ 3 ||
        throw(ArgumentError("prog: member and limit hold N values each"))
    opts = MadsOpts(poll_vars)
    g = granularity === nothing ? nothing : mesh_granularity(granularity, length(x0))
    n_p = poll_vars == :xy ? 2 * (length(x0) ÷ 3) : length(x0)
    lo, hi = shard === nothing ? (0, 2 * n_p) : shard
    prm = Ref(MadsParams(n_iter, ell0, ell_max, UInt64(seed)))
    pprev = prev === nothing ? Ptr{Float64}(C_NULL) : pointer(prev)
    pdlim = d_lim === nothing ? Ptr{Float64}(C_NULL) : pointer(d_lim)
    rcons = cons === nothing ? nothing : Ref(cons)
    rmot = motion === nothing ? nothing : Ref(CMotion(motion))
    rmesh = g === nothing ? nothing : Ref(MacMadsMesh(pointer(g), 0))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve prev d_lim motion g prog rcons rmot rmesh begin
        pcons = rcons === nothing ? Ptr{MacCons}(C_NULL) : Base.unsafe_convert(Ptr{MacCons}, rcons)
        pmot = rmot === nothing ? Ptr{CMotion}(C_NULL) : Base.unsafe_convert(Ptr{CMotion}, rmot)
        pmesh = rmesh === nothing ? Ptr{MacMadsMesh}(C_NULL) : Base.unsafe_convert(Ptr{MacMadsMesh}, rmesh)
        cp = Ref(CProg(pointer(prog.member), pointer(prog.limit), prog.n_cons, Int32(0), prog.h_max0))
        check(ccall((:mac_mads_begin_prog, libmaxcover), Int32,
                    (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64},
                     Float64, Ref{MadsParams}, Int64, Int64, Ref{Ptr{Cvoid}}, Ptr{MacCons}, Ref{MadsOpts},
                     Ptr{CMotion}, Ptr{MacMadsMesh}, Ref{CProg}),
                    ctx, x0, length(x0), r_max, penalty, pprev, pdlim, tan_half_fov, prm, lo, hi, h,
                    pcons, Ref(opts), pmot, pmesh, cp))
    end
    return MadsProgStepper(h[], ctx, length(x0))
end

"poll_prog!(st, ahead = 0) — mac_mads_poll_prog: (done, part) of the stepper's shard, `ahead` chaining iterations on."
function poll_prog!(st::MadsProgStepper, ahead::Integer = 0)
    done = Ref{Int32}(0)
    part = Ref{MacProgPart}()
    check(ccall((:mac_mads_poll_prog, libmaxcover), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{MacProgPart}),
                st.handle, ahead, done, part))
    return done[] != 0, part[]
end

"prog_merge(parts) — mac_prog_merge: the records of one iteration merged (exact, in any order; no context)."
function prog_merge(parts::Vector{MacProgPart})
    out = Ref{MacProgPart}()
    check(ccall((:mac_prog_merge, libmaxcover), Int32, (Ptr{MacProgPart}, Int32, Ref{MacProgPart}),
                parts, length(parts), out))
    return out[]
end

"advance_prog!(st, merged) — mac_mads_advance_prog: (outcome 0 / 1 / 2, chains::Bool)."
function advance_prog!(st::MadsProgStepper, merged::MacProgPart)
    outcome = Ref{Int32}(0)
    chains = Ref{Int32}(0)
    check(ccall((:mac_mads_advance_prog, libmaxcover), Int32,
                (Ptr{Cvoid}, Ref{MacProgPart}, Ref{Int32}, Ref{Int32}), st.handle, Ref(merged), outcome, chains))
    return outcome[], chains[] != 0
end

"result_prog(st) — mac_mads_result_prog: (x, stats::MadsStats, x_infeasible or nothing, pstats::MadsProgStats)."
function result_prog(st::MadsProgStepper)
    x = Vector{Float64}(undef, st.n)
    xi = fill(NaN, st.n)
    s = Ref{MadsStats}()
    ps = Ref{MadsProgStats}()
    check(ccall((:mac_mads_result_prog, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ref{MadsStats}, Ref{MadsProgStats}),
                st.handle, x, xi, s, ps))
    return x, s[], (ps[].has_infeasible != 0 ? xi : nothing), ps[]
end

"close_prog!(st) — mac_mads_destroy."
function close_prog!(st::MadsProgStepper)
    if st.handle != C_NULL
        ccall((:mac_mads_destroy, libmaxcover), Cvoid, (Ptr{Cvoid},), st.handle)
        st.handle = C_NULL
    end
    return nothing
end

"""
rmvCoveredPOI!(cells, circles) — src/CellFunctions.jl:81-108: delete, order-preserving, every
entry of cells.points_of_interest covered by `circles`; the device list is updated in place.
"""
function rmvCoveredPOI!(cells, circles::Vector{Float64}; ctx::MacContext = default_context())
    pts = cells.points_of_interest
    set_points!(ctx, pts)
    kept = Vector{Int64}(undef, length(pts))
    M = Ref{Int64}(0)
    check(ccall((:mac_remove_covered_f64, libmaxcover), Int32,
                (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ref{Int64}),
                ctx, circles, length(circles), kept, M))
    cells.points_of_interest = pts[kept[1:M[]] .+ 1]
    return cells
end

end # module
