// meao_k_downsample.hip -- the stand-alone downsample pass (the four point-sampled levels; meao_dev_downsample.hpp).
#include "meao_dev_downsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

// ROWS = kMipRowsPerLane: tiles of 128 x 16 LowDepth1 texels.  ROWS = 1, small calls (a 1080p frame: 272 tiles of 128 x 16):
// tiles of 128 x 8, twice the workgroups, one load-compute-store round each instead of two in a row.
template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_kernel(const DownsampleArgs a)
{
    downsample_tile<VEC, DIV, ROWS>(a, blockIdx.x, blockIdx.z);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers

hipError_t launch_downsample(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (linear_depth(a.depth_format)) return launch_downsample_linear(a, frames, s, pf);
    if (downsample_pitched(a)) return launch_downsample_pitched(a, frames, s, pf);
    if (pf) return launch_downsample_frames(a, frames, s, pf);
    if (!rows_per_lane_valid(a)) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_downsample_variant(a, [&](auto v) { downsample_kernel<v.kVec, v.kDiv, v.kRows><<<grid, dim3(kThreads), 0, s>>>(a); });
}

}  // namespace meao
