// meao_k_render_frames.hip -- the render kernels with per-frame constants (meao_execute_batch_params): frame blockIdx.y's
// RenderArgs from the FrameArgs table, then the same tiles as render_kernel / render_small_kernel / render_wide_kernel.  (A
// composite waiting for a per-frame call is flushed as its own launch: there is no per-frame render_with_composite_kernel.)
#include "meao_dev_render.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

template <int AOFMT, bool RTNE, int DIV, bool EXH>
__global__ __launch_bounds__(ren_tile_w(EXH) * 4, EXH ? 1 : 8) void render_frames_kernel(const RenderArgs *t)
{
    __shared__ __attribute__((aligned(16))) float tile[kRenLdsH * (ren_tile_w(EXH) + 2 * kRenApron)];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    const RenderArgs &a = frame_block(t, frame);
    if (beyond_frame(block, a.blocks_per_frame)) return;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_tile<AOFMT, RTNE, DIV_IEEE, EXH>(a, tile, frame, block);
            return;
        }
    }
    render_tile<AOFMT, RTNE, DIV, EXH>(a, tile, frame, block);
}

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(ren_tile_w(false) * 4, 6) void render_small_frames_kernel(const RenderArgs *t)
{
    __shared__ __attribute__((aligned(16))) float tile[(kRenTileHSmall + 2 * kRenApron) * (ren_tile_w(false) + 2 * kRenApron)];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    const RenderArgs &a = frame_block(t, frame);
    if (beyond_frame(block, a.blocks_per_frame)) return;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_tile<AOFMT, RTNE, DIV_IEEE, false, NoRenderHook, kRenTileHSmall>(a, tile, frame, block);
            return;
        }
    }
    render_tile<AOFMT, RTNE, DIV, false, NoRenderHook, kRenTileHSmall>(a, tile, frame, block);
}

template <int AOFMT, bool RTNE, int DIV, bool EXH>
__global__ __launch_bounds__(kThreads) void render_wide_frames_kernel(const RenderArgs *t)
{
    __shared__ __attribute__((aligned(16))) float tile[kWideLdsH * kWideLdsW];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    const RenderArgs &a = frame_block(t, frame);
    if (beyond_frame(block, a.blocks_per_frame)) return;
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_wide_tile<AOFMT, RTNE, DIV_IEEE, EXH>(a, tile, frame, block);
            return;
        }
    }
    render_wide_tile<AOFMT, RTNE, DIV, EXH>(a, tile, frame, block);
}

}  // namespace

hipError_t launch_render_frames(const RenderArgs &a, int ao_format, int frames, hipStream_t s, const RenderArgs *pf, bool wide)
{
    const dim3 grid(a.blocks_per_frame, frames, 1), block(wide ? kThreads : ren_tile_w(a.exhaustive != 0) * 4);
    return for_column(ao_format, a, [&](auto c) {
        if (wide) {
            if (a.exhaustive) render_wide_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, true><<<grid, block, 0, s>>>(pf);
            else render_wide_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, false><<<grid, block, 0, s>>>(pf);
        } else {
            if (a.exhaustive) render_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, true><<<grid, block, 0, s>>>(pf);
            else if (a.tile_h == kRenTileHSmall) render_small_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(pf);
            else render_frames_kernel<c.kAoFmt, c.kRtne, c.kDiv, false><<<grid, block, 0, s>>>(pf);
        }
    });
}

}  // namespace meao
