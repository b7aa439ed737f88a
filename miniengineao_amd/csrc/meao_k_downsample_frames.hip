// meao_k_downsample_frames.hip -- the downsample pass with per-frame constants (meao_execute_batch_params): frame blockIdx.z's
// DownsampleArgs from the FrameArgs table (meao_kernels.hpp), then the same tile as downsample_kernel.
#include "meao_dev_downsample.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_frames_kernel(const DownsampleArgs *t)
{
    downsample_tile<VEC, DIV, ROWS>(frame_block(t, blockIdx.z), blockIdx.x, blockIdx.z);
}

template <bool VEC, int DIV>
void launch_ds_frames_t(const DownsampleArgs &a, const DownsampleArgs *pf, dim3 grid, hipStream_t s)
{
    if (a.rows_per_lane == 1) downsample_frames_kernel<VEC, DIV, 1><<<grid, dim3(kThreads), 0, s>>>(pf);
    else downsample_frames_kernel<VEC, DIV, kMipRowsPerLane><<<grid, dim3(kThreads), 0, s>>>(pf);
}

}  // namespace

hipError_t launch_downsample_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (a.rows_per_lane != 1 && a.rows_per_lane != kMipRowsPerLane) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (a.exact_rcp_div) {
        if (a.vec_ok) launch_ds_frames_t<true, DIV_EXACT_RCP>(a, pf, grid, s);
        else launch_ds_frames_t<false, DIV_EXACT_RCP>(a, pf, grid, s);
    } else {
        if (a.vec_ok) launch_ds_frames_t<true, DIV_IEEE>(a, pf, grid, s);
        else launch_ds_frames_t<false, DIV_IEEE>(a, pf, grid, s);
    }
    return hipGetLastError();
}

}  // namespace meao
