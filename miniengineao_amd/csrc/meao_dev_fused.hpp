// meao_dev_fused.hpp -- the hook through which the full-resolution upsample tile carries the next batch's downsample tile
// (meao_k_upsample_fused.hip and its per-frame form).
#pragma once

#include "meao_dev_upsample.hpp"
#include "meao_dev_downsample.hpp"

namespace meao {
namespace {

// Hook of the fused last kernel: puts the two 16-byte depth loads of the carried (lean) downsample tile in flight inside the
// upsample tile, before its bilateral phase -- after the tile's own hoisted operands have landed, so that nothing in the
// bilateral phase waits behind them (vmcnt retires in order) -- to be consumed after it (A/B against "tile first" and "after
// the prefetch": profiles/r02_ab_v15p..v17p_split_ds*.jsonl).
// PITCHED: the carried frames' depth rows are d.depth_pitch texels apart (meao_k_pitched_fused*.hip).
template <bool PITCHED>
struct IssueCarriedLoadsLeanT {
    static constexpr bool kBeforeBilateral = true;
    // Forms of the bilateral texel (A/B with the whole-tile copy of the phase, profiles/r04_ab_fused_bilateral_forms.jsonl; before that
    // copy existed both lost here): exact sequences 272 us, UNORM8 estimate 257, grouped reciprocals 264, both 256 us per 16 frames.
    static constexpr bool kReuseEstimate = false;        // (round 6, with registers to spare: 240.1 vs 240.3 us -- the exact path is rare; left off)
    const DownsampleArgs &d;
    float4v (&q)[2];
    bool mine, full;
    int tile, frame;
    __device__ __forceinline__ void before_bilateral() const
    {
        if (!mine) return;
        if (full) downsample_lean_load<true, PITCHED>(d, tile, frame, q);
        else downsample_lean_load<false, PITCHED>(d, tile, frame, q);
    }
};
typedef IssueCarriedLoadsLeanT<false> IssueCarriedLoadsLean;

}  // namespace
}  // namespace meao
