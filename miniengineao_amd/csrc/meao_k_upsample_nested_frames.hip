// meao_k_upsample_nested_frames.hip -- the nested blend launches (two-level, three-level) with per-frame constants
// (meao_execute_batch_params): frame blockIdx.z's UpsampleArgs of every pass from the FrameArgs table.
#include "meao_dev_blend.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 8) void upsample_two_level_frames_kernel(const UpsampleArgs *t_outer, const UpsampleArgs *t_inner)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<NestedForm>::kFloats];
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x), frame = blockIdx.z;
    const UpsampleArgs &outer = frame_block(t_outer, frame), &inner = frame_block(t_inner, frame);
    if (beyond_frame(tile, outer.tiles_x * outer.tiles_y)) return;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(outer.hostile, outer.generation, frame)) {
            upsample_two_level_tile<AOFMT, RTNE, DIV_IEEE>(outer, inner, smem, tile, frame);
            return;
        }
    }
    upsample_two_level_tile<AOFMT, RTNE, DIV>(outer, inner, smem, tile, frame);
}

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads) void upsample_three_level_frames_kernel(const UpsampleArgs *t_outer, const UpsampleArgs *t_mid,
                                                                               const UpsampleArgs *t_inner)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<NestedForm>::kFloats + kNestScratch];
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x), frame = blockIdx.z;
    const UpsampleArgs &outer = frame_block(t_outer, frame), &mid = frame_block(t_mid, frame), &inner = frame_block(t_inner, frame);
    if (beyond_frame(tile, outer.tiles_x * outer.tiles_y)) return;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(outer.hostile, outer.generation, frame)) {
            upsample_three_level_tile<AOFMT, RTNE, DIV_IEEE>(outer, mid, inner, smem, tile, frame);
            return;
        }
    }
    upsample_three_level_tile<AOFMT, RTNE, DIV>(outer, mid, inner, smem, tile, frame);
}

// two-level: t_mid == nullptr
hipError_t launch_nested_frames(const UpsampleArgs &outer, int ao_format, int frames, hipStream_t s, const UpsampleArgs *t_outer,
                                const UpsampleArgs *t_mid, const UpsampleArgs *t_inner)
{
    const dim3 grid(outer.tiles_x * outer.tiles_y, 1, frames);
    return for_column(ao_format, outer, [&](auto c) {
        if (t_mid) upsample_three_level_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(t_outer, t_mid, t_inner);
        else upsample_two_level_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(t_outer, t_inner);
    });
}

}  // namespace

hipError_t launch_upsample_two_level_frames(const UpsampleArgs &outer, int ao_format, int frames, hipStream_t s,
                                            const UpsampleArgs *pf_outer, const UpsampleArgs *pf_inner)
{
    if (!pf_outer || !pf_inner) return hipErrorInvalidValue;
    return launch_nested_frames(outer, ao_format, frames, s, pf_outer, nullptr, pf_inner);
}

hipError_t launch_upsample_three_level_frames(const UpsampleArgs &outer, int ao_format, int frames, hipStream_t s,
                                              const UpsampleArgs *pf_outer, const UpsampleArgs *pf_mid, const UpsampleArgs *pf_inner)
{
    if (!pf_outer || !pf_mid || !pf_inner) return hipErrorInvalidValue;
    return launch_nested_frames(outer, ao_format, frames, s, pf_outer, pf_mid, pf_inner);
}

}  // namespace meao
