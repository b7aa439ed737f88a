// meao_k_pitched_fused.hip -- the full-resolution upsample carrying the next batch's downsample pass (meao_k_upsample_fused.hip)
// for row-pitched surfaces: either side -- this batch's depth and results, the next batch's depth -- may be pitched; the strides
// of a packed side are its packed rows.  Shared and per-frame forms.
#include "meao_dev_fused.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_pitched_kernel(const UpsampleArgs a, const HiDepthArgs hi,
                                                                                               const DownsampleArgs d)
{
    typedef FinalForm<ups_tile_h(true), RawDepth::F32, Rows::Pitched> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLeanT<true> issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue, &hi);
    if (mine) {
        if (full) downsample_lean_finish<DIV, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false>(d, blockIdx.x, blockIdx.z, q);
    }
}

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_pitched_frames_kernel(
    const UpsampleArgs *ta, const HiDepthArgs *th, const DownsampleArgs *td)
{
    typedef FinalForm<ups_tile_h(true), RawDepth::F32, Rows::Pitched> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(ta, blockIdx.z);
    const DownsampleArgs &d = frame_block(td, blockIdx.z);
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLeanT<true> issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue,
                                                          &frame_block(th, blockIdx.z));
    if (mine) {
        if (full) downsample_lean_finish<DIV, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false>(d, blockIdx.x, blockIdx.z, q);
    }
}

}  // namespace

// (the caller has checked fused_downsample_applicable; every stride of the blocks is set: packed sides carry their packed rows)
hipError_t launch_upsample_final_with_downsample_pitched(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int ao_format,
                                                         int frames, hipStream_t s, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                                         const DownsampleArgs *pf_d)
{
    if (!final_strides_set(a) || !depth_stride_set(d) || !all_or_none(pf, pf_hi, pf_d)) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames), block(kThreads);
    return for_column(ao_format, a, [&](auto c) {
        if (pf) upsample_final_with_next_downsample_pitched_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(pf, pf_hi, pf_d);
        else upsample_final_with_next_downsample_pitched_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(a, hi, d);
    });
}

}  // namespace meao
