// meao_k_linear_frames.hip -- the linear-depth kernels (meao_k_linear.hip) with per-frame constants (meao_execute_batch_params):
// frame blockIdx.z's argument blocks from the FrameArgs table, whose zp0 is that frame's s.
#include "meao_dev_downsample.hpp"
#include "meao_dev_upsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_linear_frames_kernel(const DownsampleArgs *t)
{
    const DownsampleArgs &a = frame_block(t, blockIdx.z);
    if (beyond_frame(blockIdx.x, a.tiles_x * a.tiles_y)) return;
    downsample_tile<VEC, DIV, ROWS, true, true>(a, blockIdx.x, blockIdx.z);
}

template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_linear_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    typedef FinalForm<ups_tile_h(true), RawDepth(F32), Rows::Pitched, DepthKind::Linear> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z, NoHook(), &frame_block(th, blockIdx.z));
}

template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_linear_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    typedef FinalForm<kUpsTileHSmall, RawDepth(F32), Rows::Pitched, DepthKind::Linear> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z, NoHook(), &frame_block(th, blockIdx.z));
}

}  // namespace

hipError_t launch_downsample_linear_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_downsample_variant(a, [&](auto v) { downsample_linear_frames_kernel<v.kVec, v.kDiv, v.kRows><<<grid, dim3(kThreads), 0, s>>>(pf); });
}

hipError_t launch_upsample_final_linear_frames(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                               const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (!pf_hi) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        for_final_variant<MEAO_DEPTH_LINEAR_F32>(a, hi, [&](auto v) {
            if constexpr (v.kSmall) upsample_final_small_linear_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(pf, pf_hi);
            else upsample_final_linear_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(pf, pf_hi);
        });
    });
}

}  // namespace meao
