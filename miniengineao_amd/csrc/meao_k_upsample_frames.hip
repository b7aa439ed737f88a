// meao_k_upsample_frames.hip -- the upsample kernels with per-frame constants (meao_execute_batch_params): frame blockIdx.z's
// UpsampleArgs (and HiDepthArgs) from the FrameArgs table, then the same tiles as upsample_kernel / upsample_final_kernel /
// upsample_final_small_kernel / upsample_blend_tall_kernel.
#include "meao_dev_upsample.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 1) void upsample_frames_kernel(const UpsampleArgs *t)
{
    typedef BlendForm<> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z);
}

template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads, RAW_F32 ? 7 : 6) void upsample_final_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    typedef FinalForm<ups_tile_h(true), RawDepth(RAW_F32)> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z, NoHook(), &frame_block(th, blockIdx.z));
}

template <int AOFMT, bool RTNE, int DIV, bool RAW_F32>
__global__ __launch_bounds__(kThreads) void upsample_final_small_frames_kernel(const UpsampleArgs *t, const HiDepthArgs *th)
{
    typedef FinalForm<kUpsTileHSmall, RawDepth(RAW_F32)> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z, NoHook(), &frame_block(th, blockIdx.z));
}

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 6) void upsample_blend_tall_frames_kernel(const UpsampleArgs *t)
{
    typedef BlendForm<kUpsTileHTall> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(t, blockIdx.z);
    const int tile = xcd_contiguous(blockIdx.x, gridDim.x);
    if (beyond_frame(tile, a.tiles_x * a.tiles_y)) return;
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, tile, blockIdx.z);
}

}  // namespace

// hi: the shared HiDepthArgs of a final pass (selects the raw-format kernel), nullptr = a blend pass; pf_hi: the frames' blocks
hipError_t launch_upsample_frames(const UpsampleArgs &a, const HiDepthArgs *hi, int ao_format, int frames, hipStream_t s,
                                  const UpsampleArgs *pf, const HiDepthArgs *pf_hi)
{
    if (hi && !pf_hi) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        if (hi) {
            for_final_variant<MEAO_DEPTH_F32>(a, *hi, [&](auto v) {
                if constexpr (v.kSmall) upsample_final_small_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(pf, pf_hi);
                else upsample_final_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, v.kF32><<<grid, block, 0, s>>>(pf, pf_hi);
            });
        } else if (a.tile_h == kUpsTileHTall) {
            upsample_blend_tall_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(pf);
        } else {
            upsample_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(pf);
        }
    });
}

}  // namespace meao
