// meao_k_upsample_fused.hip -- the full-resolution upsample kernel that carries the next batch's downsample pass (meao_prefetch_batch).
#include "meao_dev_fused.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

// Upsample.main of this batch carrying the downsample pass of the NEXT batch (meao_prefetch_batch).  The carried pass is pure
// streaming with ~2 VALU instructions per byte; inside this kernel its traffic overlaps the arithmetic of the other resident
// workgroups instead of costing a launch of its own between two VALU-bound ones.  Since round 6 both halves move fewer bytes:
// the pass writes the four levels only (it reads the even rows of the next frames: 27.6 MB per 4K frame instead of 60.8) and the
// upsample tile linearizes its HiResDB from the raw depth of ITS frames (33.2 MB read instead of 16.6 written + 16.6 read back).
// One lean downsample tile (64 x 16 LowDepth1 texels) per upsample tile (64 x 64): d.tiles_x * d.tiles_y <= gridDim.x
// (fused_downsample_applicable); each workgroup puts its tile's loads in flight inside its upsample tile and finishes it after.
template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(kThreads, 7) void upsample_final_with_next_downsample_kernel(const UpsampleArgs a, const HiDepthArgs hi,
                                                                                       const DownsampleArgs d)
{
    typedef FinalForm<> Form;
    __shared__ __attribute__((aligned(16))) float smem[UpsLds<Form>::kFloats];
    const bool mine = blockIdx.x < static_cast<unsigned>(d.tiles_x * d.tiles_y) && blockIdx.z < static_cast<unsigned>(d.frames);
    float4v q[2];
    const bool full = (static_cast<int>(blockIdx.x) / d.tiles_x + 1) * kLeanRows <= d.h[1];
    const IssueCarriedLoadsLean issue = {d, q, mine, full, static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.z)};
    upsample_tile_checked<Column<AOFMT, RTNE, DIV>, Form>(a, smem, xcd_contiguous(blockIdx.x, gridDim.x), blockIdx.z, issue, &hi);
    if (mine) {
        if (full) downsample_lean_finish<DIV, true>(d, blockIdx.x, blockIdx.z, q);
        else downsample_lean_finish<DIV, false>(d, blockIdx.x, blockIdx.z, q);
    }
    // (loading the carried tile behind the first barrier and finishing it in FRONT of the bilateral phase frees its VGPRs there
    // and is 5 % slower: profiles/r03_ab_fused_ds_finished_before_bilateral.jsonl)
}


}  // namespace

// ------------------------------------------------------------------------------------------
// launchers

// The fused form needs f32 depth on both sides, frames the 16-byte loads of the lean tile apply to (d.vec_ok: W % 8 == 0, aligned)
// and a grid that has a workgroup for every carried tile.  `d` must be tiled for the lean tile: tiles of kLeanW x kLeanRows.
bool fused_downsample_applicable(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int frames)
{
    // (f32 depth: the raw format, or linear view-space depth -- meao_k_linear_fused.hip)
    const bool f32 = (hi.depth_format == MEAO_DEPTH_F32 && d.depth_format == MEAO_DEPTH_F32) ||
                     (hi.depth_format == MEAO_DEPTH_LINEAR_F32 && d.depth_format == MEAO_DEPTH_LINEAR_F32);
    return f32 && d.vec_ok != 0 && a.tile_h == ups_tile_h(true) &&
           d.tiles_x * d.tiles_y <= a.tiles_x * a.tiles_y && d.frames <= frames;
}

hipError_t launch_upsample_final_with_downsample(const UpsampleArgs &a, const HiDepthArgs &hi, const DownsampleArgs &d, int ao_format,
                                                 int frames, hipStream_t s, const UpsampleArgs *pf, const HiDepthArgs *pf_hi,
                                                 const DownsampleArgs *pf_d)
{
    if (!fused_downsample_applicable(a, hi, d, frames)) return hipErrorInvalidValue;      // the caller asks first
    if (linear_depth(hi.depth_format)) return launch_upsample_final_with_downsample_linear(a, hi, d, ao_format, frames, s, pf, pf_hi, pf_d);
    if (final_pitched(a) || downsample_pitched(d))
        return launch_upsample_final_with_downsample_pitched(a, hi, d, ao_format, frames, s, pf, pf_hi, pf_d);
    if (pf || pf_hi || pf_d) return launch_upsample_final_with_downsample_frames(a, ao_format, frames, s, pf, pf_hi, pf_d);
    const dim3 grid(a.tiles_x * a.tiles_y, 1, frames);
    return for_column(ao_format, a, [&](auto c) {
        upsample_final_with_next_downsample_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, dim3(kThreads), 0, s>>>(a, hi, d);
    });
}

}  // namespace meao
