// meao_k_pitched.hip -- the kernels that address caller memory, for row-pitched surfaces (meao_execute_batch_pitched): the
// stand-alone downsample pass and the full-resolution upsample (64 x 64 and small tiles).  The same device functions as
// meao_k_downsample.hip / meao_k_upsample.hip with PITCHED set: the raw depth rows are DownsampleArgs::depth_pitch /
// UpsampleArgs::pitch.depth texels apart and the result rows UpsampleArgs::pitch.dst.  Units of their own, so that the packed
// kernels compile exactly as they would without them.
#include "meao_dev_downsample.hpp"
#include "meao_dev_upsample.hpp"
#include "meao_launch.hpp"

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
    typedef FinalForm<ups_tile_h(true), RawDepth(RAW_F32), Rows::Pitched> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_pitched_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    typedef FinalForm<kUpsTileHSmall, RawDepth(RAW_F32), Rows::Pitched> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

}  // namespace

hipError_t launch_downsample_pitched(const DownsampleArgs &a, int frames, hipStream_t s, const DownsampleArgs *pf)
{
    if (!rows_per_lane_valid(a) || !depth_stride_set(a)) return hipErrorInvalidValue;
    if (pf) return launch_downsample_pitched_frames(a, frames, s, pf);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_downsample_variant(a, [&](auto v) { downsample_pitched_kernel<v.kVec, v.kDiv, v.kRows><<<grid, dim3(kThreads), 0, s>>>(a); });
}

hipError_t launch_upsample_final_pitched(const UpsampleArgs &a, const HiDepthArgs &hi, int ao_format, int frames, hipStream_t s,
                                         const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (!final_strides_set(a)) return hipErrorInvalidValue;     // both strides are set in a pitched call
    if (pf) return launch_upsample_final_pitched_frames(a, hi, ao_format, frames, s, pf, pf_hi);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        for_final_variant<MEAO_DEPTH_F32>(a, hi, [&](auto v) {
            if constexpr (v.kSmall) upsample_final_small_pitched_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, hi);
            else upsample_final_pitched_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, hi);
        });
    });
}

}  // namespace meao
