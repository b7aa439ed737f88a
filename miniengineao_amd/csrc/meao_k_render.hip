// meao_k_render.hip -- render kernels: interleaved (all levels, one grid), small tiles, wide (Render.main), and the form that carries a composite.
#include "meao_dev_render.hpp"
#include "meao_dev_composite.hpp"
#include "meao_launch.hpp"

namespace meao {
namespace {

// 128 x 32 tiles: 40 KB window, 4 workgroups of 8 waves per CU = 8 waves per SIMD (<= 64 VGPRs).
template <int AOFMT, bool RTNE, int DIV, bool EXH>
__global__ __launch_bounds__(ren_tile_w(EXH) * 4, EXH ? 1 : 8) void render_kernel(const RenderArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[kRenLdsH * (ren_tile_w(EXH) + 2 * kRenApron)];
#if MEAO_X_PHASE_CLOCKS
    const unsigned long long wg_t0 = __builtin_amdgcn_s_memrealtime();      // every wave: the first one in and the last one out are logged
#endif
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {       // wave-uniform, decided per frame
            render_tile<AOFMT, RTNE, DIV_IEEE, EXH>(a, tile, frame, block);
            return;
        }
    }
    render_tile<AOFMT, RTNE, DIV, EXH>(a, tile, frame, block);
#if MEAO_X_PHASE_CLOCKS
    const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
    if ((threadIdx.x & 63) == 0 && id < 16384) {
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        atomicMin(&g_wg_log[id * 4 + 0], wg_t0);           // earliest wave start (the host presets ~0)
        atomicMax(&g_wg_log[id * 4 + 1], t1);              // latest wave end
        atomicMin(&g_wg_log[id * 4 + 2], t1);              // earliest wave end: the skew inside the workgroup
        if (threadIdx.x == 0)
            g_wg_log[id * 4 + 3] = (__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)) & 0xFu) |
                                   (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11))) << 8);
    }
#endif
}

// (128 x 64 tiles with 1024 threads -- a 60 KB window, two workgroups = 32 waves per CU, apron share 1.875x instead of 2.5x, half
// the hand-overs per texel -- measured 170.2 vs 166.2 us per 16 frames at 4K, profiles/r04_ab_render_tile_128x64.jsonl: the
// barrier of sixteen waves and a hand-over that idles half a CU cost more than the smaller apron saves.  With 96 x 32 (r03),
// 64 x 32 (r01) and the dynamic blocks (r03) that closes the tile-shape question: render runs at 2.98 cycles per VALU
// instruction, the hand-over of a full CU's LDS is what separates it from the 2.4-2.55 of its loop, and no shape removes it.
// Nor does taking the hand-over away: persistent 1024-thread workgroups whose four loader waves fill the next tile's window while
// twelve compute waves evaluate the current one (two window buffers, one barrier per tile) run at 209-220 us -- the barrier of
// sixteen waves per tile costs more than the hand-over did: profiles/r04_ab_render_producer_consumer.jsonl.)
// One or two small frames per call (fewer 128 x 32 tiles than CUs): 128 x 8 tiles, four times the workgroups,
// one texel-loop iteration each -- the call waits for one workgroup's serial time, not for throughput.
template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(ren_tile_w(false) * 4, 6) void render_small_kernel(const RenderArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[(kRenTileHSmall + 2 * kRenApron) * (ren_tile_w(false) + 2 * kRenApron)];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_tile<AOFMT, RTNE, DIV_IEEE, false, NoRenderHook, kRenTileHSmall>(a, tile, frame, block);
            return;
        }
    }
    render_tile<AOFMT, RTNE, DIV, false, NoRenderHook, kRenTileHSmall>(a, tile, frame, block);
}

// Render.main (WIDE_SAMPLING): render_wide_tile, meao_dev_render.hpp.
template <int AOFMT, bool RTNE, int DIV, bool EXH>
__global__ __launch_bounds__(kThreads) void render_wide_kernel(const RenderArgs a)
{
    __shared__ __attribute__((aligned(16))) float tile[kWideLdsH * kWideLdsW];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_wide_tile<AOFMT, RTNE, DIV_IEEE, EXH>(a, tile, frame, block);
            return;
        }
    }
    render_wide_tile<AOFMT, RTNE, DIV, EXH>(a, tile, frame, block);
}

// The render pass carrying the composite of frames that an EARLIER call produced (meao_composite_enqueue):
// the composite is pure streaming (17 bytes per texel, as many bytes as the whole AO path) and render
// is VALU-bound with HBM nearly idle, so every render workgroup first streams its share of the
// composite texel pairs and then renders its tile.
// carried composite (multiply mode): two pixel pairs per lane in flight under every texel-loop iteration (three: 0.830 vs 0.834 ms, not kept)
constexpr int kCompositePerIteration = 2;
constexpr int kCompositePairsInLoop = kCompositePerIteration * (kRenTileH / 8);
constexpr int kCarriedThreads = ren_tile_w(false) * 4;          // the workgroup of render_with_composite_kernel

// Pass 2 of Blit.shader (dst * src.a) for pixel pairs of ONE frame, as the hook of the render texel loop:
// begin(k) issues the 16-byte colour and 2/4-byte AO loads of two pairs, end(k) multiplies and stores them.
// Slot j of a lane is pair q = q0 + j * q_step: its colour 16 q bytes from `color`, its AO j * ao_step bytes behind the lane's first
// AO pair; taken while q < full_pairs (0: the loop takes nothing).  j < kCompositePairsInLoop here, the rest in the plain loop
// before the tile.
// Packed: q = (j * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x, the pair index in the frame (a workgroup touches 8 KB of
// contiguous colour per j), ao_step = q_step pairs of AO, full_pairs = the pairs of the frame with both pixels.
// Row-pitched (meao_composite_enqueue_pitched; vector-eligible surfaces only, so a colour row is a whole number of 16-byte steps):
// a row is 2^L chunks of kCarriedThreads pairs and workgroup b of the first G = gridDim.x & ~(2^L - 1) owns chunk b mod 2^L of the
// rows (b >> L) + j * (G >> L).  `color` and `ao` point at that chunk in its first row, q0 = the lane, q_step = the 16-byte steps
// and ao_step the bytes from one of its rows to the next, full_pairs = q_step * its rows within the slots; a lane beyond the row's
// full pairs gets a q0 no slot takes.  So both layouts are the same loop code and the same six words of state (one in a VGPR).
template <int AOFMT>
struct CarriedComposite {
    typedef AoTexel<AOFMT> AO;
    const typename AO::type *ao;
    uint16_t *color;
    uint32_t q0, q_step, ao_step, full_pairs;
    static constexpr uint32_t kNoPair = 0x80000000u;      // as q0: no slot is below full_pairs (q_step < 2^28 where it is set, so nothing wraps)
    uint4v col[kCompositePerIteration];
    typedef typename std::conditional<sizeof(typename AO::type) == 1, uint16_t, uint32_t>::type ao_pair_bits;
    uint32_t ao2[kCompositePerIteration];     // two AO texels, undecoded (taken apart in end(), not next to the load)
    __device__ __forceinline__ uint32_t pair_of(int k, int s) const { return q0 + static_cast<uint32_t>(kCompositePerIteration * k + s) * q_step; }
    __device__ __forceinline__ uint32_t ao_offset(int k, int s) const
    {
        return q0 * static_cast<uint32_t>(sizeof(ao_pair_bits)) + static_cast<uint32_t>(kCompositePerIteration * k + s) * ao_step;
    }
    __device__ __forceinline__ void begin(int k)
    {
#pragma unroll
        for (int s = 0; s < kCompositePerIteration; ++s) {
            const uint32_t q = pair_of(k, s);
            if (q < full_pairs) {
                col[s] = __builtin_nontemporal_load(reinterpret_cast<const uint4v *>(at_byte_offset(color, q * 16u)));
                ao2[s] = *reinterpret_cast<const ao_pair_bits *>(at_byte_offset(ao, ao_offset(k, s)));
            }
        }
        __builtin_amdgcn_sched_barrier(0);        // the loads stay here; their first use is behind the texel arithmetic
    }
    __device__ __forceinline__ void end(int k)
    {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < kCompositePerIteration; ++s) {
            const uint32_t q = pair_of(k, s);
            if (q < full_pairs) {
                constexpr int kAoBits = 8 * sizeof(typename AO::type);
                asm volatile("" : "+v"(ao2[s]));          // opaque here: nothing derived from the loaded word moves up to the load
                const float a0 = AO::decode(static_cast<typename AO::type>(ao2[s] & ((1u << kAoBits) - 1u)));
                const float a1 = AO::decode(static_cast<typename AO::type>(ao2[s] >> kAoBits));
                const uint32_t w[4] = {col[s].x, col[s].y, col[s].z, col[s].w};
                uint32_t o[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) {                      // words 0, 1: pixel 0 (rg, ba); words 2, 3: pixel 1
                    const float m = h < 2 ? a0 : a1;
                    const uint32_t lo = f32_to_f16_rtne_bits(f16_bits_to_f32(static_cast<uint16_t>(w[h] & 0xffffu)) * m);
                    const uint32_t hi = f32_to_f16_rtne_bits(f16_bits_to_f32(static_cast<uint16_t>(w[h] >> 16)) * m);
                    o[h] = lo | (hi << 16);
                }
                __builtin_nontemporal_store(uint4v{o[0], o[1], o[2], o[3]}, reinterpret_cast<uint4v *>(at_byte_offset(color, q * 16u)));
            }
        }
    }
};

template <int AOFMT, bool RTNE, int DIV>
__global__ __launch_bounds__(ren_tile_w(false) * 4, 8) void render_with_composite_kernel(const RenderArgs a,
                                                                                         const CompositeBatchArgs c)
{
    __shared__ __attribute__((aligned(16))) float tile[kRenLdsH * (ren_tile_w(false) + 2 * kRenApron)];
    const int frame = blockIdx.y, block = xcd_contiguous(blockIdx.x, gridDim.x);
    // In-loop form: one composite frame per render frame, multiply mode, frames below 2^28 pairs (32-bit byte offsets)
    const bool in_loop = c.mode == MEAO_COMPOSITE_MULTIPLY && c.frames == static_cast<int32_t>(gridDim.y) &&
                         c.pixels < (int64_t(1) << 29);
    CarriedComposite<AOFMT> carried;
    typedef typename CarriedComposite<AOFMT>::ao_pair_bits ao_pair_bits;
    carried.ao = static_cast<const typename AoTexel<AOFMT>::type *>(c.ao[frame]);
    carried.color = static_cast<uint16_t *>(c.color[frame]);
    carried.q0 = carried.q_step = carried.ao_step = carried.full_pairs = 0;       // the loop takes nothing
    if (__builtin_expect(!c.pitch.on, 1)) {     // tightly packed: laid out first
        if (in_loop) {
            const int64_t pairs = (c.pixels + 1) / 2;
            carried.q_step = gridDim.x * blockDim.x;
            carried.ao_step = carried.q_step * static_cast<uint32_t>(sizeof(ao_pair_bits));
            carried.q0 = blockIdx.x * blockDim.x + threadIdx.x;
            carried.full_pairs = static_cast<uint32_t>(c.pixels / 2);
            // what the loop does not take: pairs j >= kCompositePairsInLoop of this lane and the half pair of an odd frame
            for (int64_t q = static_cast<int64_t>(carried.q0) + static_cast<int64_t>(kCompositePairsInLoop) * carried.q_step; q < pairs; q += carried.q_step)
                composite_pair<AOFMT>(c.ao[frame], c.color[frame], c.gbuffer0[frame], c.pixels, c.mode, q);
            if (c.pixels & 1) {     // the half pair at the end of an odd frame: the lane that owns it, if the loop would have had it
                const int64_t last = pairs - 1;
                if (last % carried.q_step == carried.q0 && last / carried.q_step < kCompositePairsInLoop)
                    composite_pair<AOFMT>(c.ao[frame], c.color[frame], c.gbuffer0[frame], c.pixels, c.mode, last);
            }
        } else {
            const int64_t pairs = (c.pixels + 1) / 2, total = pairs * c.frames;
            const int64_t stride = static_cast<int64_t>(gridDim.x) * gridDim.y * blockDim.x;
            for (int64_t i = (static_cast<int64_t>(blockIdx.y) * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
                const int f = static_cast<int>(i / pairs);
                composite_pair<AOFMT>(c.ao[f], c.color[f], c.gbuffer0[f], c.pixels, c.mode, i - f * pairs);
            }
        }
    } else {                // kernel-uniform: row-pitched surfaces
        const CompositePitches &p = c.pitch;
        const uint32_t row_pairs = (static_cast<uint32_t>(p.w) + 1u) / 2u, h = static_cast<uint32_t>(p.h);
        if (in_loop) {
            typedef typename AoTexel<AOFMT>::type ao_t;
            const uint32_t lg = static_cast<uint32_t>(c.chunks_log2), mask = (1u << lg) - 1u;
            const uint32_t owners = gridDim.x & ~mask;          // at least 2^L (the launcher's choice of L); the others only render
            if (blockIdx.x < owners) {
                const uint32_t chunk = blockIdx.x & mask, row0 = blockIdx.x >> lg, row_step = owners >> lg;
                const uint32_t px0 = chunk * kCarriedThreads + threadIdx.x, row_full = p.vec ? static_cast<uint32_t>(p.w) / 2u : 0u;
                // what the loop does not take: rows beyond its slots, pairs beyond the 2^L chunks, half pairs, and every pair of a
                // scalar-form surface
                uint32_t mine = 0;
                for (uint32_t row = row0; row < h; row += row_step, ++mine) {
                    for (uint32_t px = px0; px < row_pairs; px += static_cast<uint32_t>(kCarriedThreads) << lg) {
                        const bool slot = mine < static_cast<uint32_t>(kCompositePairsInLoop) && px == px0 && px < row_full;
                        if (!slot) composite_pair<AOFMT>(c.ao[frame], c.color[frame], c.gbuffer0[frame], p, c.mode, row, px);
                    }
                }
                if (row_full != 0) {        // vector-eligible: p.color is even
                    const uint32_t chunk_pair = chunk * kCarriedThreads;
                    carried.ao = at_byte_offset(carried.ao, (__umul24(row0, p.ao) + 2u * chunk_pair) * static_cast<uint32_t>(sizeof(ao_t)));
                    carried.color = at_byte_offset(carried.color, (__umul24(row0, p.color) + 2u * chunk_pair) * 8u);
                    carried.q0 = px0 < row_full ? threadIdx.x : CarriedComposite<AOFMT>::kNoPair;
                    // Two rows of a frame are less than 2^32 bytes apart (meao_composite_enqueue_pitched), so with a second row
                    // q_step < 2^28 and no q wraps, kNoPair's included; the owner of one row never steps, and any q_step from
                    // the row's full pairs up serves it.  __umul24: row_step <= 32768, the limit of a configuration's extent
                    // (config_valid), and a pitch is below 2^24 texels.
                    carried.q_step = mine > 1 ? __umul24(row_step, p.color >> 1) : row_full;
                    carried.ao_step = __umul24(row_step, p.ao) * static_cast<uint32_t>(sizeof(ao_t));
                    carried.full_pairs = min(mine, static_cast<uint32_t>(kCompositePairsInLoop)) * carried.q_step;
                }
            }
        } else {
            const uint32_t units = h * static_cast<uint32_t>(c.frames);        // (frame, row), dealt to all workgroups of the grid
            for (uint32_t u = blockIdx.y * gridDim.x + blockIdx.x; u < units; u += gridDim.x * gridDim.y) {
                const uint32_t f = u / h;
                composite_row<AOFMT>(c.ao[f], c.color[f], c.gbuffer0[f], p, c.mode, u - f * h, threadIdx.x, kCarriedThreads);
            }
        }
    }
    if constexpr (DIV == DIV_EXACT_RCP) {
        if (frame_is_hostile(a.hostile, a.generation, frame)) {
            render_tile<AOFMT, RTNE, DIV_IEEE, false>(a, tile, frame, block, carried);
            return;
        }
    }
    render_tile<AOFMT, RTNE, DIV, false>(a, tile, frame, block, carried);
}


}  // namespace

// ------------------------------------------------------------------------------------------
// launchers

// WIDE selects render_wide_kernel; the exhaustive / small-tile choice inside the column
template <bool WIDE>
static hipError_t launch_render_any(const RenderArgs &a, int ao_format, int frames, hipStream_t s)
{
    const dim3 grid(a.blocks_per_frame, frames, 1), block(WIDE ? kThreads : ren_tile_w(a.exhaustive != 0) * 4);
    return for_column(ao_format, a, [&](auto c) {
        if constexpr (WIDE) {
            if (a.exhaustive) render_wide_kernel<c.kAoFmt, c.kRtne, c.kDiv, true><<<grid, block, 0, s>>>(a);
            else render_wide_kernel<c.kAoFmt, c.kRtne, c.kDiv, false><<<grid, block, 0, s>>>(a);
        } else {
            if (a.exhaustive) render_kernel<c.kAoFmt, c.kRtne, c.kDiv, true><<<grid, block, 0, s>>>(a);
            else if (a.tile_h == kRenTileHSmall) render_small_kernel<c.kAoFmt, c.kRtne, c.kDiv><<<grid, block, 0, s>>>(a);
            else render_kernel<c.kAoFmt, c.kRtne, c.kDiv, false><<<grid, block, 0, s>>>(a);
        }
    });
}

hipError_t launch_render(const RenderArgs &a, int ao_format, int frames, hipStream_t s, const RenderArgs *pf)
{
    if (pf) return launch_render_frames(a, ao_format, frames, s, pf, false);
    return launch_render_any<false>(a, ao_format, frames, s);
}

hipError_t launch_render_with_composite(const RenderArgs &a, const CompositeBatchArgs &batch, int ao_format, int frames, hipStream_t s)
{
    if (a.exhaustive) return hipErrorInvalidValue;     // the 68-sample variant keeps its own launch; the caller flushes instead
    CompositeBatchArgs c = batch;
    c.chunks_log2 = 0;      // a row as 2^L chunks of a workgroup's lanes: the least L that spans its pairs, at most 3 and 2^L workgroups
    while ((kCarriedThreads << c.chunks_log2) < (c.pitch.w + 1) / 2 && c.chunks_log2 < 3 && (a.blocks_per_frame >> (c.chunks_log2 + 1)) > 0)
        ++c.chunks_log2;
    const dim3 grid(a.blocks_per_frame, frames, 1);
    return for_column(ao_format, a, [&](auto col) {
        render_with_composite_kernel<col.kAoFmt, col.kRtne, col.kDiv><<<grid, dim3(kCarriedThreads), 0, s>>>(a, c);
    });
}

hipError_t launch_render_wide(const RenderArgs &a, int ao_format, int frames, hipStream_t s, const RenderArgs *pf)
{
    if (pf) return launch_render_frames(a, ao_format, frames, s, pf, true);
    return launch_render_any<true>(a, ao_format, frames, s);
}

}  // namespace meao
