// meao_k_downsample_frames.hip -- the downsample pass with per-frame constants (meao_execute_batch_params): frame blockIdx.z's
// DownsampleArgs from the FrameArgs table (meao_kernels.hpp), then the same tile as downsample_kernel.
#include "meao_dev_downsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_frames_kernel(const DownsampleArgs *t)
{
    const DownsampleArgs &a = frame_block(t, blockIdx.z);
    if (beyond_frame(blockIdx.x, a.tiles_x * a.tiles_y)) return;
    downsample_tile<VEC, DIV, ROWS>(a, blockIdx.x, blockIdx.z);
}

}  // namespace

hipError_t launch_downsample_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (!rows_per_lane_valid(a)) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_downsample_variant(a, [&](auto v) { downsample_frames_kernel<v.kVec, v.kDiv, v.kRows><<<grid, dim3(kThreads), 0, s>>>(pf); });
}

}  // namespace meao
