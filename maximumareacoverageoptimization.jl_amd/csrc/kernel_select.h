// kernel_select.h — host only: the instantiation a launch takes, as its kernel pointer. The template
// arguments are the launches' compile-time switches; every combination named here is one the library
// builds, and none is built that is not named here. Included by maxcover.hip after kernels.h, its
// `using namespace mac` and eval_plan.h (PrepKind).
#pragma once

#include <type_traits>

// UAVs per thread of the constraint kernels (k_cons.h cons_slots: 1, 2, 4, 8) as a template argument:
// pick(std::integral_constant<int, S>) returns that instantiation
template <class F>
static auto by_slots(int S, F pick)
{
    return S == 1 ? pick(std::integral_constant<int, 1>{}) : S == 2 ? pick(std::integral_constant<int, 2>{})
         : S == 4 ? pick(std::integral_constant<int, 4>{}) : pick(std::integral_constant<int, 8>{});
}

using MaskKern = void (*)(const double*, int, ConsArgs, uint8_t*);
using MaskMotionKern = void (*)(const double*, int, ConsArgs, MotionArgs, uint8_t*);
using MaskGenKern = void (*)(uint64_t*, CandSrc, int, ConsArgs, uint8_t*);
using MaskGenMotionKern = void (*)(uint64_t*, CandSrc, int, ConsArgs, MotionArgs, uint8_t*);

static MaskKern mask_kern(int S)
{
    return by_slots(S, [](auto v) -> MaskKern { return cons_mask_kernel<decltype(v)::value>; });
}

// (under a mac_motion: with d_sep off, the kernels without the sort and its LDS arrays)
static MaskMotionKern mask_motion_kern(int S, bool sep)
{
    return sep ? by_slots(S, [](auto v) -> MaskMotionKern { return cons_mask_motion_kernel<decltype(v)::value, true>; })
               : by_slots(S, [](auto v) -> MaskMotionKern { return cons_mask_motion_kernel<decltype(v)::value, false>; });
}

static MaskGenKern mask_gen_kern(int S)
{
    return by_slots(S, [](auto v) -> MaskGenKern { return cons_mask_gen_kernel<decltype(v)::value>; });
}

static MaskGenMotionKern mask_gen_motion_kern(int S, bool sep)
{
    return sep ? by_slots(S, [](auto v) -> MaskGenMotionKern { return cons_mask_gen_motion_kernel<decltype(v)::value, true>; })
               : by_slots(S, [](auto v) -> MaskGenMotionKern { return cons_mask_gen_motion_kernel<decltype(v)::value, false>; });
}

// the sort's LDS of a mask launch: x, y, cell per sorted position
static uint32_t mask_lds(int S) { return (uint32_t)(17 * kConsBlock * S); }

// the verdict launches (k_cons.h cons_explain): sep selects the build with the sort; its LDS adds each
// position's UAV index (2 B) and its "in a pair" byte
using ExplainKern = void (*)(const double*, int, ExplainArgs, Verdict*);
using ExplainGenKern = void (*)(uint64_t*, CandSrc, int, ExplainArgs, Verdict*, unsigned long long*);
static ExplainKern explain_kern(int S, bool sep)
{
    return sep ? by_slots(S, [](auto v) -> ExplainKern { return cons_explain_kernel<decltype(v)::value, true>; })
               : by_slots(S, [](auto v) -> ExplainKern { return cons_explain_kernel<decltype(v)::value, false>; });
}
static ExplainGenKern explain_gen_kern(int S, bool sep)
{
    return sep ? by_slots(S, [](auto v) -> ExplainGenKern { return cons_explain_gen_kernel<decltype(v)::value, true>; })
               : by_slots(S, [](auto v) -> ExplainGenKern { return cons_explain_gen_kernel<decltype(v)::value, false>; });
}
static uint32_t explain_lds(int S, bool sep) { return sep ? (uint32_t)(20 * kConsBlock * S) : 0u; }

// (a mesh belongs to a generated poll: prep_x_kernel's matrix build has none)
using PrepKern = void (*)(uint64_t*, PrepArgs);
// (mesh: EvalPlan.mesh, the kMesh argument: 0 none, 1 a mesh with value keys, kMeshKeys)
static PrepKern prep_kern(int kind, int mesh)
{
    if (kind == kPrepXGen)
        return mesh == kMeshKeys ? prep_x_kernel<true, kMeshKeys> : mesh ? prep_x_kernel<true, 1> : prep_x_kernel<true>;
    if (kind == kPrepXMatrix) return prep_x_kernel<false>;
    return mesh == kMeshKeys ? prep_kernel<kMeshKeys> : mesh ? prep_kernel<1> : prep_kernel<0>;
}
static dim3 prep_block(int kind) { return dim3(kind == kPrepChains ? kPrepU : kPrepU + kWave); }

// (an xy-only poll's and a mesh's kernels are their own instantiations: the full poll's stay as they were)
using IdxKern = void (*)(uint64_t*, CandSrc, int, int, Grid, int, IndexOut);
template <bool kKeys, int kPer>
static IdxKern index_kern_of(bool xy, int mesh)
{
    return mesh == kMeshKeys ? (xy ? disk_index_kernel<kKeys, kPer, true, kMeshKeys> : disk_index_kernel<kKeys, kPer, false, kMeshKeys>)
         : mesh ? (xy ? disk_index_kernel<kKeys, kPer, true, 1> : disk_index_kernel<kKeys, kPer, false, 1>)
                : (xy ? disk_index_kernel<kKeys, kPer, true> : disk_index_kernel<kKeys, kPer>);
}
static IdxKern index_kern(bool keys, bool wide, bool xy, int mesh)
{
    return keys ? (wide ? index_kern_of<true, kIdxPerWide>(xy, mesh) : index_kern_of<true, kIdxPer>(xy, mesh))
                : (wide ? index_kern_of<false, kIdxPerWide>(xy, mesh) : index_kern_of<false, kIdxPer>(xy, mesh));
}

// the source selects the instantiation of the fused chain's launches (k_fiw.h kMat): a matrix poll's
// has no generator code in it; generated and basis-form polls take the other (kXY, kMesh: theirs only)
using FiwKern = void (*)(uint64_t*, FwArgs);
template <bool kCounts>
static FiwKern fiw_kern_of(bool mat, int mesh)
{
    return mat ? fiw_kernel<kCounts, true>
         : mesh == kMeshKeys ? fiw_kernel<kCounts, false, kMeshKeys>
         : mesh ? fiw_kernel<kCounts, false, 1> : fiw_kernel<kCounts, false>;
}
static FiwKern fiw_kern(bool counts, bool mat, int mesh)
{
    return counts ? fiw_kern_of<true>(mat, mesh) : fiw_kern_of<false>(mat, mesh);
}

using Fin2Kern = void (*)(const unsigned*, const double*, int, int, int, double, const double*, double*, double*,
                          FinBest, F2Shared, uint64_t*);
template <bool kCounts>
static Fin2Kern fin2_kern_of(bool mat, bool xy, int mesh)
{
    return mat ? fin2_kernel<kCounts, true>
         : mesh == kMeshKeys ? (xy ? fin2_kernel<kCounts, false, true, kMeshKeys> : fin2_kernel<kCounts, false, false, kMeshKeys>)
         : mesh ? (xy ? fin2_kernel<kCounts, false, true, 1> : fin2_kernel<kCounts, false, false, 1>)
         : xy ? fin2_kernel<kCounts, false, true> : fin2_kernel<kCounts, false>;
}
static Fin2Kern fin2_kern(bool counts, bool mat, bool xy, int mesh)
{
    return counts ? fin2_kern_of<true>(mat, xy, mesh) : fin2_kern_of<false>(mat, xy, mesh);
}

using FinKern = void (*)(const double*, const int*, int, int, int, int, const int*, const double*, const int*, int,
                         double, const double*, double*, double*, FinBest, uint64_t*);
static FinKern finalize_kern(bool xy, bool mesh)
{
    return mesh ? (xy ? finalize_kernel<true, true> : finalize_kernel<false, true>)
                : xy ? finalize_kernel<true> : finalize_kernel<false>;
}
