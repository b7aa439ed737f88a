// meao_k_upsample_fused_frames.hip -- the full-resolution upsample kernel carrying the next batch's downsample pass, with
// per-frame constants (meao_execute_batch_params / meao_prefetch_batch_params): frame blockIdx.z's table entry holds this
// batch's frame for the upsample tile and the next batch's frame blockIdx.z for the carried tile.
#include "meao_dev_fused.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_frames_kernel(const UpsampleArgs *ta, const HiDepthArgs *th,
                                                                                              const DownsampleArgs *td)
{
    typedef FinalForm<> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const UpsampleArgs &a = frame_block(ta, blockIdx.z);
    const DownsampleArgs &d = frame_block(td, blockIdx.z);
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLean issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue,
                                                          &frame_block(th, blockIdx.z));
    if (mine) {
        if (full) downsample_lean_finish<DIV, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false>(d, blockIdx.x, blockIdx.z, q);
    }
}

}  // namespace

// (the caller has checked fused_downsample_applicable on the shared blocks: the geometry is the same in every frame)
hipError_t launch_upsample_final_with_downsample_frames(const UpsampleArgs &a, int ao_format, int frames, hipStream_t s,
                                                        const UpsampleArgs *pf, const HiDepthArgs *pf_hi, const DownsampleArgs *pf_d)
{
    if (!pf || !pf_hi || !pf_d) return hipErrorInvalidValue;
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_column(ao_format, a, [&](auto c) {
        upsample_final_with_next_downsample_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(pf, pf_hi, pf_d);
    });
}

}  // namespace meao
