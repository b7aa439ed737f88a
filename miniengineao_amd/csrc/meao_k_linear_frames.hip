// meao_k_linear_frames.hip -- the linear-depth kernels (meao_k_linear.hip) with per-frame constants (meao_execute_batch_params):
// frame blockIdx.z's argument blocks from the FrameArgs table, whose zp0 is that frame's s.
#include "meao_dev_downsample.hpp"
#include "meao_dev_upsample.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_linear_frames_kernel(const DownsampleArgs *t)
{
    downsample_tile<VEC, DIV, ROWS, true, true>(frame_block(t, blockIdx.z), blockIdx.x, blockIdx.z);
}

template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_linear_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true>::kFloats];
    upsample_tile_checked<AOFMT, RTNE, true, DIV, NoHook, ups_tile_h(true), F32, true, true>(frame_block(t, blockIdx.z), smem,
                                                                                          xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z,
                                                                                          NoHook(), &frame_block(th, blockIdx.z));
}

template <int AOFMT, bool RTNE, int DIV, bool F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_linear_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true, kUpsTileHSmall>::kFloats];
    upsample_tile_checked<AOFMT, RTNE, true, DIV, NoHook, kUpsTileHSmall, F32, true, true>(frame_block(t, blockIdx.z), smem,
                                                                                        xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z,
                                                                                        NoHook(), &frame_block(th, blockIdx.z));
}

template <bool VEC, int DIV>
void launch_ds_linear_frames_t(const DownsampleArgs &a, const DownsampleArgs *pf, dim3 grid, hipStream_t s)
{
    if (a.rows_per_lane == 1) downsample_linear_frames_kernel<VEC, DIV, 1><<<grid, dim3(kThreads), 0, s>>>(pf);
    else downsample_linear_frames_kernel<VEC, DIV, kMipRowsPerLane><<<grid, dim3(kThreads), 0, s>>>(pf);
}

template <int AOFMT, bool RTNE, int DIV>
void launch_final_linear_frames_t(const UpsampleArgs &a, const HiDepthArgs &hi, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                  dim3 grid, hipStream_t s)
{
    const dim3 block(kThreads);
    const bool f32 = hi.depth_format == MEAO_DEPTH_LINEAR_F32;
    if (a.tile_h == kUpsTileHSmall) {
        if (f32) upsample_final_small_linear_frames_kernel<AOFMT, RTNE, DIV, true><<<grid, block, 0, s>>>(pf, pf_hi);
        else upsample_final_small_linear_frames_kernel<AOFMT, RTNE, DIV, false><<<grid, block, 0, s>>>(pf, pf_hi);
    } else {
        if (f32) upsample_final_linear_frames_kernel<AOFMT, RTNE, DIV, true><<<grid, block, 0, s>>>(pf, pf_hi);
        else upsample_final_linear_frames_kernel<AOFMT, RTNE, DIV, false><<<grid, block, 0, s>>>(pf, pf_hi);
    }
}

}  // namespace

hipError_t launch_downsample_linear_frames(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (a.exact_rcp_div) {
        if (a.vec_ok) launch_ds_linear_frames_t<true, DIV_EXACT_RCP>(a, pf, grid, s);
        else launch_ds_linear_frames_t<false, DIV_EXACT_RCP>(a, pf, grid, s);
    } else {
        if (a.vec_ok) launch_ds_linear_frames_t<true, DIV_IEEE>(a, pf, grid, s);
        else launch_ds_linear_frames_t<false, DIV_IEEE>(a, pf, grid, s);
    }
    return hipGetLastError();
}

hipError_t launch_upsample_final_linear_frames(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                               const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (!pf_hi) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (ao_format == MEAO_AO_R8) {
        if (a.f16_rtne) launch_final_linear_frames_t<MEAO_AO_R8, true, DIV_IEEE>(a, hi, pf, pf_hi, grid, s);
        else if (a.exact_rcp_div) launch_final_linear_frames_t<MEAO_AO_R8, false, DIV_EXACT_RCP>(a, hi, pf, pf_hi, grid, s);
        else launch_final_linear_frames_t<MEAO_AO_R8, false, DIV_IEEE>(a, hi, pf, pf_hi, grid, s);
    } else {
        if (a.f16_rtne) launch_final_linear_frames_t<MEAO_AO_F16, true, DIV_IEEE>(a, hi, pf, pf_hi, grid, s);
        else if (a.exact_rcp_div) launch_final_linear_frames_t<MEAO_AO_F16, false, DIV_EXACT_RCP>(a, hi, pf, pf_hi, grid, s);
        else launch_final_linear_frames_t<MEAO_AO_F16, false, DIV_IEEE>(a, hi, pf, pf_hi, grid, s);
    }
    return hipGetLastError();
}

}  // namespace meao
