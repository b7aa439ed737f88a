// meao_k_linear_fused.hip -- the full-resolution upsample carrying the next batch's downsample pass (meao_k_upsample_fused.hip) for
// linear view-space f32 depth (MEAO_DEPTH_LINEAR_F32): this batch's HiResDB and the carried tile's levels are linearize_view of
// the frames (zp0 = s), the LoResDB interior comes from registers as in the raw form.  Rows through the pitch fields, like every
// linear kernel.  Shared and per-frame forms.
#include "meao_dev_fused.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_linear_kernel(const UpsampleArgs a, const HiDepthArgs hi,
                                                                                              const DownsampleArgs d)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true>::kFloats];
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLeanT<true> issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<AOFMT, RTNE, true, DIV, IssueCarriedLoadsLeanT<true>, ups_tile_h(true), true, true, true>(
        a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue, &hi);
    if (mine) {
        if (full) downsample_lean_finish<DIV, true, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false, true>(d, blockIdx.x, blockIdx.z, q);
    }
}

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_linear_frames_kernel(
    const UpsampleArgs *ta, const HiDepthArgs *th, const DownsampleArgs *td)
{
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<true>::kFloats];
    const UpsampleArgs &a = frame_block(ta, blockIdx.z);
    const DownsampleArgs &d = frame_block(td, blockIdx.z);
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLeanT<true> issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<AOFMT, RTNE, true, DIV, IssueCarriedLoadsLeanT<true>, ups_tile_h(true), true, true, true>(
        a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue, &frame_block(th, blockIdx.z));
    if (mine) {
        if (full) downsample_lean_finish<DIV, true, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false, true>(d, blockIdx.x, blockIdx.z, q);
    }
}

template <int AOFMT, bool RTNE, int DIV>
void launch_fused_linear_t(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, const UpsampleArgs *pf,
                           const HiDepthArgs *pf_hi, const DownsampleArgs *pf_d, dim3 grid, hipStream_t s)
{
    if (pf) upsample_final_with_next_downsample_linear_frames_kernel<AOFMT, RTNE, DIV><<<grid, dim3(kThreads), 0, s>>>(pf, pf_hi, pf_d);
    else upsample_final_with_next_downsample_linear_kernel<AOFMT, RTNE, DIV><<<grid, dim3(kThreads), 0, s>>>(a, hi, d);
}

}  // namespace

// (the caller has checked fused_downsample_applicable; every stride of the blocks is set: packed sides carry their packed rows)
hipError_t launch_upsample_final_with_downsample_linear(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int ao_format,
                                                        int frames, hipStream_t s, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                                        const DownsampleArgs *pf_d)
{
    if (hi.depth_format != MEAO_DEPTH_LINEAR_F32 || d.depth_format != MEAO_DEPTH_LINEAR_F32) return hipErrorInvalidValue;
    if (a.pitch.depth < a.hw || a.pitch.dst < a.hw || d.depth_pitch < d.w[0]) return hipErrorInvalidValue;
    if ((pf || pf_hi || pf_d) && !(pf && pf_hi && pf_d)) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    if (ao_format == MEAO_AO_R8) {
        if (a.f16_rtne) launch_fused_linear_t<MEAO_AO_R8, true, DIV_IEEE>(a, hi, d, pf, pf_hi, pf_d, grid, s);
        else if (a.exact_rcp_div) launch_fused_linear_t<MEAO_AO_R8, false, DIV_EXACT_RCP>(a, hi, d, pf, pf_hi, pf_d, grid, s);
        else launch_fused_linear_t<MEAO_AO_R8, false, DIV_IEEE>(a, hi, d, pf, pf_hi, pf_d, grid, s);
    } else {
        if (a.f16_rtne) launch_fused_linear_t<MEAO_AO_F16, true, DIV_IEEE>(a, hi, d, pf, pf_hi, pf_d, grid, s);
        else if (a.exact_rcp_div) launch_fused_linear_t<MEAO_AO_F16, false, DIV_EXACT_RCP>(a, hi, d, pf, pf_hi, pf_d, grid, s);
        else launch_fused_linear_t<MEAO_AO_F16, false, DIV_IEEE>(a, hi, d, pf, pf_hi, pf_d, grid, s);
    }
    return hipGetLastError();
}

}  // namespace meao
