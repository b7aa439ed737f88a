// meao_k_upsample_nested.hip -- blend passes evaluated inside the launch of the pass above them (two-level, three-level).
#include "meao_dev_blend.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

// Upsample.main_blendout L4 -> L3 evaluated inside the L3 -> L2 pass (upsample_two_level_tile, meao_dev_blend.hpp).
template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 8) void upsample_two_level_kernel(const UpsampleArgs outer, const UpsampleArgs inner)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<NestedForm>::kFloats];
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x), frame = blockIdx.z;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(outer.hostile, outer.generation, frame)) {
            upsample_two_level_tile<AOFMT, RTNE, DIV_IEEE>(outer, inner, smem, tile, frame);
            return;
        }
    }
    upsample_two_level_tile<AOFMT, RTNE, DIV>(outer, inner, smem, tile, frame);
}

// One or two frames per call: L4 -> L3 and L3 -> L2 inside the L2 -> L1 launch (upsample_three_level_tile, meao_dev_blend.hpp).
template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads) void upsample_three_level_kernel(const UpsampleArgs outer, const UpsampleArgs mid,
                                                                        const UpsampleArgs inner)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<NestedForm>::kFloats + kNestScratch];
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x), frame = blockIdx.z;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(outer.hostile, outer.generation, frame)) {
            upsample_three_level_tile<AOFMT, RTNE, DIV_IEEE>(outer, mid, inner, smem, tile, frame);
            return;
        }
    }
    upsample_three_level_tile<AOFMT, RTNE, DIV>(outer, mid, inner, smem, tile, frame);
}


}  // namespace

// ------------------------------------------------------------------------------------------
// launchers

hipError_t launch_upsample_two_level(const UpsampleArgs &outer, const UpsampleArgs &inner, int ao_format, int frames, hipStream_t s,
                                     const UpsampleArgs *pf_outer, const UpsampleArgs *pf_inner)
{
    if (pf_outer || pf_inner) return launch_upsample_two_level_frames(outer, ao_format, frames, s, pf_outer, pf_inner);
    const dim3 grid(outer.tiles_x * outer.tiles_y, 1, frames);
    return for_column(ao_format, outer, [&](auto c) {
        upsample_two_level_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(outer, inner);
    });
}

hipError_t launch_upsample_three_level(const UpsampleArgs &outer, const UpsampleArgs &mid, const UpsampleArgs &inner, int ao_format,
                                       int frames, hipStream_t s, const UpsampleArgs *pf_outer, const UpsampleArgs *pf_mid,
                                       const UpsampleArgs *pf_inner)
{
    if (pf_outer || pf_mid || pf_inner) return launch_upsample_three_level_frames(outer, ao_format, frames, s, pf_outer, pf_mid, pf_inner);
    const dim3 grid(outer.tiles_x * outer.tiles_y, 1, frames);
    return for_column(ao_format, outer, [&](auto c) {
        upsample_three_level_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(outer, mid, inner);
    });
}

}  // namespace meao
