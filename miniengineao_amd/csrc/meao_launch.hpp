// meao_launch.hpp -- the launch layer the kernel units (meao_k_*.hip) share: which instantiation a set of arguments selects, the
// argument checks in front of a launch, and the launchers by which one unit hands a pass to another.  Host code only.  The units
// exist to keep the device code of the kernel families apart; every selection rule is written here, once.
#pragma once

// A host unit of the C ABI layer (meao_execute.cpp) defines MEAO_LAUNCH_RULES_ONLY in front of this header: it gets the rules
// that are plain functions of the argument blocks and none of the device headers (its translation unit holds no device code).
#ifdef MEAO_LAUNCH_RULES_ONLY
#include "meao_kernels.hpp"
#else
#include "meao_dev.hpp"
#endif

namespace meao {

// ---------------------------------------------------------------------------------------
// Hand-offs between units.  The launchers of meao_kernels.hpp take every form of a pass and hand it on: to the linear units
// when the depth is linear, else to the pitched units when a caller-memory stride is not the packed one, else to the per-frame
// units when a table is given, else they launch the shared kernel themselves.

// Pitched surfaces (meao_execute_batch_pitched): a pass whose caller-memory row strides differ from the packed ones runs the
// pitched instance of its kernel (meao_k_pitched*.hip); a stride of 0 or of the packed row means packed.
inline bool downsample_pitched(const DownsampleArgs &d) { return d.depth_pitch != 0 && d.depth_pitch != d.w[0]; }
inline bool final_pitched(const UpsampleArgs &a)
{
    return (a.pitch.depth != 0 && a.pitch.depth != a.hw) || (a.pitch.dst != 0 && a.pitch.dst != a.hw);
}

// The per-frame forms (meao_k_*_frames.hip).  `a` / `outer` select the kernel and the grid; every argument block comes from the
// table.
hipError_t launch_downsample_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf);
hipError_t launch_render_frames(const RenderArgs &a, int ao_format, int frames, hipStream_t s, const RenderArgs *pf, bool wide);
hipError_t launch_upsample_frames(const UpsampleArgs &a, const HiDepthArgs *hi, int ao_format, int frames, hipStream_t s,
                                  const UpsampleArgs *pf, const HiDepthArgs *pf_hi);
hipError_t launch_upsample_two_level_frames(const UpsampleArgs &outer, int ao_format, int frames, hipStream_t s,
                                            const UpsampleArgs *pf_outer, const UpsampleArgs *pf_inner);
hipError_t launch_upsample_three_level_frames(const UpsampleArgs &outer, int ao_format, int frames, hipStream_t s,
                                              const UpsampleArgs *pf_outer, const UpsampleArgs *pf_mid, const UpsampleArgs *pf_inner);
hipError_t launch_upsample_final_with_downsample_frames(const UpsampleArgs &a, int ao_format, int frames, hipStream_t s,
                                                        const UpsampleArgs *pf, const HiDepthArgs *pf_hi, const DownsampleArgs *pf_d);
// The pitched forms (meao_k_pitched*.hip); pf != nullptr selects the per-frame kernels.  Every stride of the blocks must be set
// (a packed side carries its packed row).
hipError_t launch_downsample_pitched(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf);
hipError_t launch_downsample_pitched_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf);
hipError_t launch_upsample_final_pitched(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                         const UpsampleArgs *pf, const HiDepthArgs *pf_hi);
hipError_t launch_upsample_final_pitched_frames(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                                const UpsampleArgs *pf, const HiDepthArgs *pf_hi);
hipError_t launch_upsample_final_with_downsample_pitched(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int ao_format,
                                                         int frames, hipStream_t s, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                                         const DownsampleArgs *pf_d);
// Linear view-space depth (MEAO_DEPTH_LINEAR_F32 / _F16; meao_k_linear*.hip).  Linear01 = z * s with s = RN(1 / far_clip) in the
// zp0 field of DownsampleArgs / HiDepthArgs / LinearDepthArgs (zp1 and reversed_z are not read).  The linear kernels always
// address the depth and result rows through the pitch fields (a packed side carries its packed row): one instance serves packed
// and pitched calls.  pf != nullptr selects the per-frame kernels.
hipError_t launch_downsample_linear(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf);
hipError_t launch_downsample_linear_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf);
hipError_t launch_upsample_final_linear(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                        const UpsampleArgs *pf, const HiDepthArgs *pf_hi);
hipError_t launch_upsample_final_linear_frames(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                               const UpsampleArgs *pf, const HiDepthArgs *pf_hi);
hipError_t launch_upsample_final_with_downsample_linear(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int ao_format,
                                                        int frames, hipStream_t s, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                                        const DownsampleArgs *pf_d);
hipError_t launch_linear_depth_view(const LinearDepthArgs &a, hipStream_t s);     // LinearDepth (debug id 1) of the linear formats

// The announced next batch's downsample pass (meao_prefetch_batch*): inside the last kernel of the carrying call, or as a launch
// of its own behind it.  `d` is the pass tiled for the lean tile, with the extents of the ANNOUNCED frames, which need not be
// those of the call (meao_prefetch_batch_sized): the carrying kernel takes the pass's geometry from `d` alone, so all it needs
// is f32 depth on both sides, the 16-byte loads (width % 8 == 0, aligned frames and pitch) and a workgroup of `a`'s grid for every
// tile of `d` -- a pass of a larger size than the call's does not fit and runs as its own launch.  own_launch:
// MEAO_DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH.
inline bool carried_in_last_kernel(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int frames, bool own_launch)
{
    return !own_launch && fused_downsample_applicable(a, hi, d, frames);
}

// ---------------------------------------------------------------------------------------
// Argument checks (a launcher that fails one returns hipErrorInvalidValue and launches nothing)

inline bool rows_per_lane_valid(const DownsampleArgs &a) { return a.rows_per_lane == 1 || a.rows_per_lane == kMipRowsPerLane; }
// the kernels that address caller memory through the pitch fields need every stride set: no 0 for "packed"
inline bool depth_stride_set(const DownsampleArgs &d) { return d.depth_pitch >= d.w[0]; }
inline bool final_strides_set(const UpsampleArgs &a) { return a.pitch.depth >= a.hw && a.pitch.dst >= a.hw; }
// the per-frame sources of a launch with several argument blocks: all of them, or none
inline bool all_or_none(const void *pf, const void *pf_hi, const void *pf_d) { return (pf && pf_hi && pf_d) || !(pf || pf_hi || pf_d); }

#ifndef MEAO_LAUNCH_RULES_ONLY
namespace {

// ---------------------------------------------------------------------------------------
// The column of a context: AO storage R8 or F16, f16 rounding, division.  `launch` is a generic callable that receives the
// column as a value whose members are constants, launch(Column<...>()): kernel<c.kAoFmt, c.kRtne, c.kDiv><<<...>>>(...).
template <int AOFMT, bool RTNE, int DIV>
struct Column {
    static constexpr int kAoFmt = AOFMT, kDiv = DIV;
    static constexpr bool kRtne = RTNE;
};

// RTNE storage always divides with IEEE '/'; the exact reciprocal sequences run with RTZ storage only: exact_rcp_div is only
// ever set together with RTZ depth storage (no inf operands), and a block that had both set would still get IEEE.  `a`: the
// argument block that carries f16_rtne and exact_rcp_div (of a nested launch: the outer pass's).
template <class Args, class Launch>
hipError_t for_column(int ao_format, const Args &a, Launch &&launch)
{
    if (ao_format == MEAO_AO_R8) {
        if (a.f16_rtne) launch(Column<MEAO_AO_R8, true, DIV_IEEE>());
        else if (a.exact_rcp_div) launch(Column<MEAO_AO_R8, false, DIV_EXACT_RCP>());
        else launch(Column<MEAO_AO_R8, false, DIV_IEEE>());
    } else {
        if (a.f16_rtne) launch(Column<MEAO_AO_F16, true, DIV_IEEE>());
        else if (a.exact_rcp_div) launch(Column<MEAO_AO_F16, false, DIV_EXACT_RCP>());
        else launch(Column<MEAO_AO_F16, false, DIV_IEEE>());
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The stand-alone downsample pass: 16-byte loads or not, division, rows per lane (rows_per_lane_valid).  The pass stores f32, so
// there is no storage rounding to choose.  launch(DownsampleVariant<...>()): kernel<v.kVec, v.kDiv, v.kRows><<<...>>>(...).
template <bool VEC, int DIV, int ROWS>
struct DownsampleVariant {
    static constexpr bool kVec = VEC;
    static constexpr int kDiv = DIV, kRows = ROWS;
};

template <class Launch>
hipError_t for_downsample_variant(const DownsampleArgs &a, Launch &&launch)
{
    const bool one = a.rows_per_lane == 1;      // else kMipRowsPerLane (rows_per_lane_valid)
    if (a.exact_rcp_div) {
        if (a.vec_ok) one ? launch(DownsampleVariant<true, DIV_EXACT_RCP, 1>()) : launch(DownsampleVariant<true, DIV_EXACT_RCP, kMipRowsPerLane>());
        else one ? launch(DownsampleVariant<false, DIV_EXACT_RCP, 1>()) : launch(DownsampleVariant<false, DIV_EXACT_RCP, kMipRowsPerLane>());
    } else {
        if (a.vec_ok) one ? launch(DownsampleVariant<true, DIV_IEEE, 1>()) : launch(DownsampleVariant<true, DIV_IEEE, kMipRowsPerLane>());
        else one ? launch(DownsampleVariant<false, DIV_IEEE, 1>()) : launch(DownsampleVariant<false, DIV_IEEE, kMipRowsPerLane>());
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// The full-resolution upsample inside a column: small tiles or 64 x 64 (two kernels, so the callable chooses between them with
// `if constexpr (v.kSmall)`), and whether the depth texels are f32 -- F32_FORMAT is the f32 member of the unit's depth formats,
// MEAO_DEPTH_F32 or MEAO_DEPTH_LINEAR_F32.
template <bool SMALL, bool F32>
struct FinalVariant {
    static constexpr bool kSmall = SMALL, kF32 = F32;
};

template <int F32_FORMAT, class Launch>
void for_final_variant(const UpsampleArgs &a, const HiDepthArgs &hi, Launch &&launch)
{
    const bool f32 = hi.depth_format == F32_FORMAT;
    if (a.tile_h == kUpsTileHSmall) {
        if (f32) launch(FinalVariant<true, true>());
        else launch(FinalVariant<true, false>());
    } else {
        if (f32) launch(FinalVariant<false, true>());
        else launch(FinalVariant<false, false>());
    }
}

}  // namespace
#endif  // MEAO_LAUNCH_RULES_ONLY
}  // namespace meao
