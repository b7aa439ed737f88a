// meao_k_upsample.hip -- upsample kernels: one blend pass / the full-resolution pass per launch.
#include "meao_dev_upsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 1) void upsample_kernel(const UpsampleArgs a)
{
    typedef BlendForm<> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z);
}

// Upsample.main: the full-resolution pass.  HiResDB comes from the caller's raw depth frames (HiDepthArgs); RAW_F32 = they are f32
// (the instance with the format switch is compiled for six workgroups per CU: its decode sequences need the registers).
template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads, RAW_F32 ? 7 : 6) void upsample_final_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    typedef FinalForm<ups_tile_h(true), RawDepth(RAW_F32)> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

// Upsample.main for calls with few tiles (one 1080p frame: 510 tiles of 64 x 64 on 256 CUs): 64 x 32 tiles, twice
// the workgroups, half the serial work in each.
template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_kernel(const UpsampleArgs a, const HiDepthArgs hi)
{
    typedef FinalForm<kUpsTileHSmall, RawDepth(RAW_F32)> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, NoHook(), &hi);
}

// Upsample.main_blendout with the full-resolution pass's 64 x 64 tiles, for launches of many tiles (L2 -> L1 of a batch: 16 320 tiles
// of 64 x 32 at 4K x 16): half the barriers and window fills per texel, apron share 1.4x instead of 1.6x; six workgroups per CU
// (23.7 KB windows, <= 80 VGPRs).  MEAO_DEBUG_BLEND_TALL_MIN_TILES.
template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 6) void upsample_blend_tall_kernel(const UpsampleArgs a)
{
    typedef BlendForm<kUpsTileHTall> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// launchers

hipError_t launch_upsample(const UpsampleArgs &a, const HiDepthArgs *hi, int ao_format, int frames, hipStream_t s,
                           const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (hi && linear_depth(hi->depth_format)) return launch_upsample_final_linear(a, *hi, ao_format, frames, s, pf, pf_hi);
    if (hi && final_pitched(a)) return launch_upsample_final_pitched(a, *hi, ao_format, frames, s, pf, pf_hi);
    if (pf) return launch_upsample_frames(a, hi, ao_format, frames, s, pf, pf_hi);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        if (hi) {
            for_final_variant<MEAO_DEPTH_F32>(a, *hi, [&](auto v) {
                if constexpr (v.kSmall) upsample_final_small_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, *hi);
                else upsample_final_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(a, *hi);
            });
        } else if (a.tile_h == kUpsTileHTall) {
            upsample_blend_tall_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(a);
        } else {
            upsample_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(a);
        }
    });
}

}  // namespace meao
