// meao_k_pitched.hip -- the kernels that address caller memory, for row-pitched surfaces (meao_execute_batch_pitched): the
// stand-alone downsample pass and the full-resolution upsample (64 x 64 and small tiles).  The same device functions as
// meao_k_downsample.hip / meao_k_upsample.hip with PITCHED set: the raw depth rows are DownsampleArgs::depth_pitch /
// UpsampleArgs::pitch.depth texels apart and the result rows UpsampleArgs::pitch.dst.  Units of their own, so that the packed
// kernels compile exactly as they would without them.
#include "meao_dev_downsample.hpp"
#include "meao_dev_upsample.hpp"

namespace meao {
namespace {

template <bool VEC, int DIV, int ROWS>
__global__ __launch_bounds__(kThreads) void downsample_pitched_kernel(const DownsampleArgs a)
{
    downsample_tile<VEC, DIV, ROWS, true>(a, blockIdx.x, blockIdx.z);
}

template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads, RAW_F32 ? 7 : 6) void upsample_final_pitched_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true>::kFloats];
    upsample_tile_checked<AOFMT, RTNE, true, DIV, NoHook, ups_tile_h(true), RAW_F32, true>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x),
                                                                                        blockIdx.z, NoHook(), &hi);
}

template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_pitched_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true, kUpsTileHSmall>::kFloats];
    upsample_tile_checked<AOFMT, RTNE, true, DIV, NoHook, kUpsTileHSmall, RAW_F32, true>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x),
                                                                                      blockIdx.z, NoHook(), &hi);
}

template <bool VEC, int DIV>
void launch_ds_pitched_t(const DownsampleArgs &a, dim3 grid, hipStream_t s)
{
    if (a.rows_per_lane == 1) downsample_pitched_kernel<VEC, DIV, 1><<<grid, dim3(kThreads), 0, s>>>(a);
    else downsample_pitched_kernel<VEC, DIV, kMipRowsPerLane><<<grid, dim3(kThreads), 0, s>>>(a);
}

template <int AOFMT, bool RTNE, int DIV>
void launch_final_pitched_t(const UpsampleArgs &a, const HiDepthArgs &hi, dim3 grid, hipStream_t s)
{
    const dim3 block(kThreads);
    const bool f32 = hi.depth_format == MEAO_DEPTH_F32;
    if (a.tile_h == kUpsTileHSmall) {
        if (f32) upsample_final_small_pitched_kernel<AOFMT, RTNE, DIV, true><<<grid, block, 0, s>>>(a, hi);
        else upsample_final_small_pitched_kernel<AOFMT, RTNE, DIV, false><<<grid, block, 0, s>>>(a, hi);
    } else {
        if (f32) upsample_final_pitched_kernel<AOFMT, RTNE, DIV, true><<<grid, block, 0, s>>>(a, hi);
        else upsample_final_pitched_kernel<AOFMT, RTNE, DIV, false><<<grid, block, 0, s>>>(a, hi);
    }
}

}  // namespace

hipError_t launch_downsample_pitched(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (a.rows_per_lane != 1 && a.rows_per_lane != kMipRowsPerLane) return hipErrorInvalidValue;
    if (a.depth_pitch < a.w[0]) return hipErrorInvalidValue;
    if (pf) return launch_downsample_pitched_frames(a, frames, s, pf);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (a.exact_rcp_div) {
        if (a.vec_ok) launch_ds_pitched_t<true, DIV_EXACT_RCP>(a, grid, s);
        else launch_ds_pitched_t<false, DIV_EXACT_RCP>(a, grid, s);
    } else {
        if (a.vec_ok) launch_ds_pitched_t<true, DIV_IEEE>(a, grid, s);
        else launch_ds_pitched_t<false, DIV_IEEE>(a, grid, s);
    }
    return hipGetLastError();
}

hipError_t launch_upsample_final_pitched(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                         const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (a.pitch.depth < a.hw || a.pitch.dst < a.hw) return hipErrorInvalidValue;     // both strides are set in a pitched call
    if (pf) return launch_upsample_final_pitched_frames(a, hi, ao_format, frames, s, pf, pf_hi);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (ao_format == MEAO_AO_R8) {
        if (a.f16_rtne) launch_final_pitched_t<MEAO_AO_R8, true, DIV_IEEE>(a, hi, grid, s);
        else if (a.exact_rcp_div) launch_final_pitched_t<MEAO_AO_R8, false, DIV_EXACT_RCP>(a, hi, grid, s);
        else launch_final_pitched_t<MEAO_AO_R8, false, DIV_IEEE>(a, hi, grid, s);
    } else {
        if (a.f16_rtne) launch_final_pitched_t<MEAO_AO_F16, true, DIV_IEEE>(a, hi, grid, s);
        else if (a.exact_rcp_div) launch_final_pitched_t<MEAO_AO_F16, false, DIV_EXACT_RCP>(a, hi, grid, s);
        else launch_final_pitched_t<MEAO_AO_F16, false, DIV_IEEE>(a, hi, grid, s);
    }
    return hipGetLastError();
}

}  // namespace meao
