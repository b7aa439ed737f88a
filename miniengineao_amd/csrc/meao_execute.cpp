// meao_execute.cpp -- the calls that launch the pipeline (meao_execute*, meao_prefetch_batch*): how a call's launch structure
// is chosen, how its kernel arguments are built, and the launch sequence of one batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "meao_ctx.hpp"
#define MEAO_LAUNCH_RULES_ONLY      // carried_in_last_kernel: the rules of the launch layer without its device headers
#include "meao_launch.hpp"

using namespace meao;

namespace {

// ------------------------------------------------------------------------------------------
// One call = plan -> launch list -> submit.  The launch structure of a batch is DATA (a LaunchList); choosing it
// (plan_launches), building the kernel arguments of a launch (ArgBuilder) and issuing it (submit_launches) are separate steps.

// What RebuildCommandBuffers records (AO.cs:511-531), in the shapes this implementation launches it in.
enum class Step {
    Downsample,               // Downsample1 + Downsample2 (AO.cs:604-658): the four levels of THIS call's frames
    Render,                   // Render.main_interleaved x levels, one grid (AO.cs:519-522)
    RenderWithComposite,      // ... carrying the composite of an earlier call's frames (meao_composite_enqueue)
    RenderHq,                 // Render.main (wide) for the levels cfg.hq_levels enables
    Blend,                    // Upsample.main_blendout writing level `hi` (AO.cs:528-530)
    BlendTwoLevel,            // L4 -> L3 evaluated inside the L3 -> L2 launch
    BlendThreeLevel,          // L4 -> L3 and L3 -> L2 evaluated inside the L2 -> L1 launch (small calls)
    Final,                    // Upsample.main: the result (AO.cs:531)
    FinalWithNextDownsample,  // ... carrying the downsample pass of the announced next batch (meao_prefetch_batch)
    DownsampleNext            // the announced batch's pass as a launch of its own behind the final one (where the fused form does not apply)
};

struct Launch {
    Step step;
    int slot;                 // meao_pass the launch is timed under; -1 = not timed
    int hi;                   // Blend*: the level written
    const char *range;        // roctx range name
};

struct LaunchList {
    Launch v[12];
    int n = 0;
    uint32_t steps = 0;       // bit per Step in the list
    void add(Step step, int slot, int hi, const char *range)
    {
        v[n++] = Launch{step, slot, hi, range};
        steps |= 1u << static_cast<int>(step);
    }
    bool has(Step step) const { return steps >> static_cast<int>(step) & 1u; }
};

struct BatchShape {           // what the structure of a call depends on
    int frames;
    bool prefetched;          // an earlier call carried this batch's downsample pass
    bool carry_composite;     // a composite batch waits for a render launch to ride in: set for a waiting RGBA16F batch ONLY (the
                              // carrying kernels read 16-byte RGBA16F pairs); a batch in another meao_color_format is flushed
                              // before the shape is filled in, and whoever fills in a BatchShape keeps that rule
    int next;                 // 0 = nothing announced; the announced pass 1 = rides in the final kernel, 2 = runs as its own launch
};

// The launch shape of one call, decided once over all its frames before any argument block is built (decide_call_shape): a
// launch runs one kernel instantiation with one tiling, so nothing that selects them may differ between the blocks of a table.
// The tile counts the thresholds compare are summed over the frames -- n x tiles where the frames have one size -- and a vector
// form needs every frame eligible by its own width, strides and pointers (a mixed call, meao_execute_batch_extents).
struct CallShape {
    int ds_rows_per_lane;         // stand-alone downsample pass: kMipRowsPerLane, or 1 (ds_small_max_tiles)
    int render_tile_h;            // interleaved checker-set render: kRenTileH, or kRenTileHSmall (render_small_max_tiles)
    int final_tile_h;             // the plain final pass: ups_tile_h(true), or kUpsTileHSmall (final_small_max_tiles)
    int blend1_tile_h;            // L2 -> L1: ups_tile_h(false), or kUpsTileHTall (blend_tall_min_tiles)
    int64_t l1_tiles;             // 64 x 32 tiles of L2 -> L1 (nested_max_tiles)
    bool ds_vec, final_vec;       // the 4-texel forms of the downsample pass and of the final pass
    int ds_rep, final_rep;        // a frame whose block selects the call's kernel: the first with a pitched depth row / a pitched
                                  // depth or result row, else frame 0
};

// l1_tiles: the call's L2 -> L1 tiles (CallShape)
LaunchList plan_launches(const meao_config &c, int64_t l1_tiles, const Tuning &t, const BatchShape &b)
{
    static const char *const kBlendRange[4] = {nullptr, "meao:upsample_L2_to_L1", "meao:upsample_L3_to_L2", "meao:upsample_L4_to_L3"};
    LaunchList l;
    if (!b.prefetched) l.add(Step::Downsample, MEAO_PASS_DOWNSAMPLE, 0, "meao:downsample");
    if (b.carry_composite) l.add(Step::RenderWithComposite, MEAO_PASS_RENDER, 0, "meao:render+composite_of_previous_call");
    else l.add(Step::Render, MEAO_PASS_RENDER, 0, "meao:render");
    if (c.hq_levels > 0) l.add(Step::RenderHq, MEAO_PASS_RENDER_HQ, 0, "meao:render_hq");
    const bool nestable = t.fuse_coarse_blend && c.num_levels == 4 && c.hq_levels == 0;
    if (nestable && l1_tiles <= t.nested_max_tiles) {
        // a small frame or two per call (at most two workgroups per CU): all three blend passes in one launch -- their latency
        // chains, not their arithmetic, are what such a call waits for (1080p: 39.2 -> 36.9 us per frame; at 4K, 1020 tiles, it
        // is a wash).  Combined3 and Combined2 are still written
        l.add(Step::BlendThreeLevel, MEAO_PASS_UPSAMPLE_1, 1, "meao:upsample_L4_to_L3+L3_to_L2+L2_to_L1");
    } else {
        // L4 -> L3 inside the L3 -> L2 launch: one launch, one latency-bound pass less (Combined3 is still written)
        if (nestable) l.add(Step::BlendTwoLevel, MEAO_PASS_UPSAMPLE_2, 2, "meao:upsample_L4_to_L3+L3_to_L2");
        else for (int hi = c.num_levels - 1; hi >= 2; --hi) l.add(Step::Blend, MEAO_PASS_UPSAMPLE_0 - hi, hi, kBlendRange[hi]);
        if (c.num_levels >= 2) l.add(Step::Blend, MEAO_PASS_UPSAMPLE_1, 1, kBlendRange[1]);
    }
    if (b.next == 1) l.add(Step::FinalWithNextDownsample, MEAO_PASS_UPSAMPLE_0, 0, "meao:upsample_L1_to_L0+downsample_next");
    else l.add(Step::Final, MEAO_PASS_UPSAMPLE_0, 0, "meao:upsample_L1_to_L0");
    // (timed in the DOWNSAMPLE slot only in calls that did not run a pass of their own there)
    if (b.next == 2) l.add(Step::DownsampleNext, b.prefetched ? MEAO_PASS_DOWNSAMPLE : -1, 0, "meao:downsample_next");
    return l;
}

// Kernel arguments of the launches of one call.
struct ArgBuilder {
    const meao_ctx *ctx;
    int n;
    const void *const *depth_dev;
    void *const *out_dev;
    const uint32_t *hostile;      // flags and generation of the downsample set this call reads
    uint32_t generation;
    const Plan *plan;             // the constants: the context's, or one frame's (meao_execute_batch_params)
    const meao_params *prm;
    int exact_rcp_div;            // of the call (over all its frames)
    int32_t depth_pitch, out_pitch;   // row strides of the depth / result frames in texels (the frames' width = packed): the call's,
                                      // or one frame's (a mixed call)
    const CallShape *shape;           // of the call

    const Plan &p() const { return *plan; }
    const meao_config &c() const { return ctx->cfg; }
    const SlotLayout &lay() const { return ctx->lay; }
    int ds_cur() const { return ctx->prefetch.ds_cur; }
    int rtne() const { return ctx->cfg.f16_rounding == MEAO_F16_RTNE; }
    // 4-texel vector loads / stores need 16-byte (f32, UNORM24), 8-byte (16-bit) aligned depth rows and 4- (R8) / 8-byte (F16)
    // aligned AO rows: width % 4 == 0 (% 8 for the downsample pass, whose lanes take 8 raw texels) and aligned base pointers
    // (include/meao.h); anything else takes the scalar variants.
    uintptr_t depth_align() const { return 4 * depth_elem(ctx->cfg.depth_format); }
    uintptr_t out_align() const { return 4 * ao_elem(ctx->cfg); }

    // ---- PushDownsampleCommands (AO.cs:604-658).  lean: tiled for the tile the final kernel carries (kLeanMipW x kLeanMipRows),
    // else for the stand-alone pass (small_ok: calls with few tiles use the one-row-per-lane tile).  own: the pass of this call's
    // own frames, whose vector form and tile come from the call's shape; null = the announced batch's pass (frames of one size)
    DownsampleArgs downsample(int frames, const void *const *depth, int32_t pitch, int set, uint32_t gen, bool lean, bool small_ok,
                              const CallShape *own = nullptr) const
    {
        DownsampleArgs ds{};
        bool aligned = (p().mip[0].w & 7) == 0 && (pitch & 3) == 0;     // (a packed row: W % 8 == 0 says it all)
        ds.depth_pitch = pitch;
        for (int f = 0; f < frames; ++f) {
            ds.depth[f] = depth[f];
            aligned = aligned && aligned_to(depth[f], depth_align());
        }
        ds.vec_ok = own ? own->ds_vec : aligned;
        ds.frames = frames;
        ds.depth_format = c().depth_format;
        for (int k = 0; k < 4; ++k) ds.low[k] = ctx->slot_ptr<float>(lay().off_low_of(set, k));
        ds.frame_stride = lay().slot_bytes;
        for (int k = 0; k < 5; ++k) { ds.w[k] = p().mip[k].w; ds.h[k] = p().mip[k].h; }
        float zc[2];
        depth_decode_constants(c().depth_format, p().zbuffer_params, *prm, zc);
        ds.zp0 = zc[0];
        ds.zp1 = zc[1];
        ds.reversed_z = prm->reversed_z != 0;
        ds.f16_rtne = rtne();
        ds.exact_rcp_div = exact_rcp_div;
        if (lean) {
            ds.rows_per_lane = 1;
            ds.tiles_x = (ds.w[1] + kLeanMipW - 1) / kLeanMipW;
            ds.tiles_y = (ds.h[1] + kLeanMipRows - 1) / kLeanMipRows;
        } else {
            ds.rows_per_lane = kMipRowsPerLane;
            ds.tiles_x = (ds.w[1] + kMipTileW - 1) / kMipTileW;
            ds.tiles_y = (ds.h[1] + kMipRowsPerPass * kMipRowsPerLane - 1) / (kMipRowsPerPass * kMipRowsPerLane);
            if (own ? own->ds_rows_per_lane == 1 : small_ok && frames * ds.tiles_x * ds.tiles_y <= ctx->tuning.ds_small_max_tiles) {
                ds.rows_per_lane = 1;
                ds.tiles_y = (ds.h[1] + kMipRowsPerPass - 1) / kMipRowsPerPass;
            }
        }
        ds.hostile = ctx->hostile_of(set);
        ds.generation = gen;
        return ds;
    }

    // ---- PushRenderCommands x num_levels (AO.cs:519-522): the levels [first, last] as one grid
    RenderArgs render(int first, int last, bool wide, bool allow_small) const
    {
        RenderArgs rn{};
        int blocks = 0, count = 0;
        // few tiles (a 1080p frame or two): 128 x 8 tiles instead of 128 x 32 (render_small_kernel)
        const int tile_h = allow_small && !wide && c().sample_set != MEAO_SAMPLES_EXHAUSTIVE ? shape->render_tile_h : kRenTileH;
        rn.tile_h = tile_h;
        for (int l = first; l <= last; ++l) {
            if (wide && !level_has_hq(c().num_levels, c().hq_levels, l)) continue;
            RenderLevelArgs &L = rn.level[count++];
            const RenderLevelPlan &rp = wide ? p().render_hq[l - 1] : p().render[l - 1];
            L.src = ctx->slot_ptr<float>(lay().off_low_of(ds_cur(), l - 1));
            L.dst = ctx->slot_ptr<void>(wide ? lay().off_hq[l - 1] : lay().off_occ[l - 1]);
            L.lw = p().mip[l].w; L.lh = p().mip[l].h;
            L.sw = p().mip[l + 2].w; L.sh = p().mip[l + 2].h;
            const int tile_w = wide ? kWideTileW : ren_tile_w(c().sample_set == MEAO_SAMPLES_EXHAUSTIVE);
            L.tiles_x = (L.lw + tile_w - 1) / tile_w;
            L.tiles_y = (L.lh + tile_h - 1) / tile_h;
            L.block_begin = blocks;
            blocks += L.tiles_x * L.tiles_y;
            L.pad_value = rp.pad_value;
            for (int t = 0; t < rp.terms; ++t) {
                L.inv_thickness[t] = rp.inv_thickness[t];
                L.front_depth[t] = rp.front_depth[t];
                L.weight[t] = rp.scaled_weight[t];
            }
            L.reject_fadeoff = rp.cb.reject_fadeoff;
            L.intensity = rp.cb.intensity;
        }
        rn.frame_stride = lay().slot_bytes;
        rn.num_levels = count;
        rn.blocks_per_frame = blocks;
        rn.f16_rtne = rtne();
        rn.exact_rcp_div = exact_rcp_div;
        rn.exhaustive = c().sample_set == MEAO_SAMPLES_EXHAUSTIVE;
        rn.hostile = hostile;
        rn.generation = generation;
        return rn;
    }

    // ---- PushUpsampleCommands (AO.cs:750-785): the pass that writes level `hi`.  carrying: the final pass of a call whose
    // last kernel carries the next batch's downsample pass (always 64 x 64 tiles)
    UpsampleArgs upsample(int hi, bool carrying = false) const
    {
        UpsampleArgs up{};
        const meao_upsample_constants &k = p().upsample[hi];   // low level = hi + 1
        up.lo_depth = ctx->slot_ptr<float>(lay().off_low_of(ds_cur(), hi));
        // LoResAO1: the coarsest level's Occlusion, else the Combined buffer of the previous pass
        up.lo_ao = ctx->slot_ptr<void>(hi == c().num_levels - 1 ? lay().off_occ[hi] : lay().off_comb[hi]);
        // main_premin*: the Render.main output of the low level is min-combined in PrefetchData
        up.lo_ao2 = level_has_hq(c().num_levels, c().hq_levels, hi + 1) ? ctx->slot_ptr<void>(lay().off_hq[hi]) : nullptr;
        up.frame_stride = lay().slot_bytes;
        up.lw = p().mip[hi + 1].w; up.lh = p().mip[hi + 1].h;
        up.hw = p().mip[hi].w; up.hh = p().mip[hi].h;
        up.tiles_x = (up.hw + kUpsTileW - 1) / kUpsTileW;
        up.tile_h = ups_tile_h(hi == 0);
        // few tiles (one 1080p frame): the plain final pass runs 64 x 32 tiles (upsample_final_small_kernel)
        if (hi == 0 && !carrying) up.tile_h = shape->final_tile_h;
        // L2 -> L1 of a large batch: 64 x 64 tiles like the full-resolution pass (upsample_blend_tall_kernel)
        if (hi == 1) up.tile_h = shape->blend1_tile_h;
        up.tiles_y = (up.hh + up.tile_h - 1) / up.tile_h;
        up.noise_filter_strength = k.noise_filter_strength;
        up.step_size = k.step_size;
        up.blur_tolerance = k.blur_tolerance;
        up.upsample_tolerance = k.upsample_tolerance;
        up.f16_rtne = rtne();
        up.exact_rcp_div = exact_rcp_div;
        up.hostile = hostile;
        up.generation = generation;
        bool vec_ok = (up.hw & 3) == 0;
        if (hi > 0) {   // main_blendout: blend with Occlusion<hi>, write Combined<hi>
            up.hi_depth = ctx->slot_ptr<float>(lay().off_low_of(ds_cur(), hi - 1));
            up.hi_ao = ctx->slot_ptr<void>(lay().off_occ[hi - 1]);
            up.dst[0] = ctx->slot_ptr<void>(lay().off_comb[hi - 1]);
        } else {        // main: HiResDB from the raw depth frames (hi_depth()), no HiResAO, write the result
            up.hi_ao = nullptr;
            up.pitch.depth = depth_pitch;      // (in place of hi_depth, which the final pass does not read)
            up.pitch.dst = out_pitch;
            vec_ok = shape->final_vec;
            for (int f = 0; f < n; ++f) up.dst[f] = out_dev[f];
        }
        up.vec_ok = vec_ok;
        return up;
    }

    // HiResDB of Upsample.main = LinearZ (DS1:37-48), which the final pass evaluates from this call's raw depth frames
    HiDepthArgs hi_depth() const
    {
        HiDepthArgs hd{};
        for (int f = 0; f < n; ++f) hd.raw[f] = depth_dev[f];
        hd.depth_format = c().depth_format;
        hd.reversed_z = prm->reversed_z != 0;
        float zc[2];
        depth_decode_constants(c().depth_format, p().zbuffer_params, *prm, zc);
        hd.zp0 = zc[0];
        hd.zp1 = zc[1];
        return hd;
    }
};

// The argument blocks of every launch of one call, built by one ArgBuilder: the context's constants (a shared call; the kernarg
// copies), or one frame's (an entry of the FrameArgs table of a per-frame call).  `nb` builds the announced batch's pass.
void build_call_args(const ArgBuilder &args, const ArgBuilder &nb, const BatchShape &b, const LaunchList &list, FrameArgs *out)
{
    const meao_ctx *ctx = args.ctx;
    const meao_config &c = ctx->cfg;
    const Prefetch &pre = ctx->prefetch;
    const int n = args.n;
    if (!b.prefetched) out->ds = args.downsample(n, args.depth_dev, args.depth_pitch, pre.ds_cur, pre.generation(), false, true, args.shape);
    out->render = args.render(1, c.num_levels, false, !b.carry_composite);
    if (c.hq_levels > 0) out->render_hq = args.render(1, c.num_levels, true, false);
    for (int hi = 1; hi < c.num_levels; ++hi) out->up[hi] = args.upsample(hi);
    if (list.has(Step::BlendThreeLevel) && out->up[1].tile_h != ups_tile_h(false)) {      // the nested launch tiles L2 -> L1 with 64 x 32
        out->up[1].tile_h = ups_tile_h(false);
        out->up[1].tiles_y = (out->up[1].hh + out->up[1].tile_h - 1) / out->up[1].tile_h;
    }
    out->up[0] = args.upsample(0, b.next == 1);
    out->hi = args.hi_depth();
    if (b.next != 0)
        out->next_ds = nb.downsample(pre.next.n, pre.next.depth, pre.next.depth_pitch, pre.other(), pre.set_gen[pre.other()], b.next == 1,
                                     b.next == 2);
}

// One batch on its way through run_batch: the device frames, and what the steps work out about them.
struct Call {
    int n;
    const void *const *depth_dev;
    void *const *out_dev;
    hipStream_t stream;
    const meao_params *fp;                // per-frame parameters (meao_execute_batch_params), nullptr = the context's
    int32_t depth_pitch, out_pitch;       // row strides of the device frames in texels (cfg.width = tightly packed)
    // A mixed call (meao_execute_batch_extents): frame f's own size, and its row strides in texels (depth_pitch / out_pitch
    // above are then unused).  null = every frame has the context's size.
    const meao_extent *extents = nullptr;
    const int32_t *depth_pitch_of = nullptr, *out_pitch_of = nullptr;
    const Plan *plan_of[MEAO_MAX_BATCH];
    const meao_params *prm_of[MEAO_MAX_BATCH];
    int exact;
    bool next_per_frame, per_frame;       // the announced batch has its own constants / the call reads a FrameArgs table
    BatchShape shape;
    CallShape launch;                     // decide_call_shape

    bool mixed() const { return extents != nullptr; }
    int32_t depth_rows(int f) const { return mixed() ? depth_pitch_of[f] : depth_pitch; }
    int32_t out_rows(int f) const { return mixed() ? out_pitch_of[f] : out_pitch; }

    // The constants the announced batch's pass is built from where it brought none of its own: the context's plan, or the plan
    // of the announced size (meao_prefetch_batch_sized).
    static const Plan *next_shared_plan(const meao_ctx *ctx)
    {
        return ctx->prefetch.next.sized ? &ctx->prefetch.next.shared_plan : &ctx->plan;
    }
    ArgBuilder builder(const meao_ctx *ctx, const Plan *plan, const meao_params *prm) const
    {
        return ArgBuilder{ctx, n, depth_dev, out_dev, ctx->hostile_of(ctx->prefetch.ds_cur), ctx->prefetch.generation(), plan, prm, exact,
                          depth_pitch, out_pitch, &launch};
    }
    // The builder of frame f's blocks: its constants and, in a mixed call, its size (the plan's) and row strides.
    ArgBuilder frame_builder(const meao_ctx *ctx, int f) const
    {
        ArgBuilder b = builder(ctx, plan_of[f], prm_of[f]);
        b.depth_pitch = depth_rows(f);
        b.out_pitch = out_rows(f);
        return b;
    }
};

// Step 1.  Constants of this call's frames: the context's plan, or each frame's own (the same plan code, so the per-frame values
// are those a shared call with that frame's parameters would use).  Exact division is chosen for the call: AND over its frames.
void resolve_constants(meao_ctx *ctx, Call *call)
{
    const meao_config &c = ctx->cfg;
    call->exact = ctx->exact_rcp_div;
    if (call->fp || call->mixed()) {      // (a mixed call: the plan of each frame's own size, the context's plan is not read)
        call->exact = 1;
        for (int f = 0; f < call->n; ++f) {
            call->prm_of[f] = call->fp ? &call->fp[f] : &ctx->prm;
            build_plan(call->mixed() ? call->extents[f].width : c.width, call->mixed() ? call->extents[f].height : c.height, c.num_levels,
                       c.sample_set, *call->prm_of[f], &ctx->frame_plan[f]);
            call->plan_of[f] = &ctx->frame_plan[f];
            if (!exact_rcp_div_applicable(c, ctx->frame_plan[f])) call->exact = 0;
        }
    } else {
        for (int f = 0; f < call->n; ++f) { call->plan_of[f] = &ctx->plan; call->prm_of[f] = &ctx->prm; }
    }
    call->next_per_frame = ctx->prefetch.next.n > 0 && ctx->prefetch.next.per_frame;
    call->per_frame = call->fp != nullptr || call->next_per_frame || call->mixed();
}

// Step 2.  The launch shape, once for the call (CallShape).  Frames of one size sum to n x tiles: what such calls always chose.
void decide_call_shape(const meao_ctx *ctx, Call *call)
{
    const meao_config &c = ctx->cfg;
    const Tuning &t = ctx->tuning;
    const uintptr_t depth_align = 4 * depth_elem(c.depth_format), out_align = 4 * ao_elem(c);
    auto tiles = [](const Dims &d, int tw, int th) { return static_cast<int64_t>((d.w + tw - 1) / tw) * ((d.h + th - 1) / th); };
    int64_t ds_tiles = 0, render_tiles = 0, final_tiles = 0, l1_tiles = 0;
    CallShape &s = call->launch;
    s.ds_vec = s.final_vec = true;
    s.ds_rep = s.final_rep = -1;
    for (int f = 0; f < call->n; ++f) {
        const Plan &p = *call->plan_of[f];
        const int32_t w = p.mip[0].w, depth_rows = call->depth_rows(f), out_rows = call->out_rows(f);
        ds_tiles += tiles(p.mip[1], kMipTileW, kMipRowsPerPass * kMipRowsPerLane);
        for (int l = 1; l <= c.num_levels; ++l) render_tiles += tiles(p.mip[l], ren_tile_w(false), kRenTileH);
        final_tiles += tiles(p.mip[0], kUpsTileW, ups_tile_h(true));
        l1_tiles += tiles(p.mip[1], kUpsTileW, ups_tile_h(false));
        // 4-texel loads / stores (ArgBuilder::depth_align): width % 8 (downsample: a lane takes 8 raw texels) or % 4, strides
        // that are multiples of 4 texels (a packed row: the width says it all), aligned frames
        const bool depth_ok = (depth_rows & 3) == 0 && aligned_to(call->depth_dev[f], depth_align);
        s.ds_vec = s.ds_vec && (w & 7) == 0 && depth_ok;
        s.final_vec = s.final_vec && (w & 3) == 0 && depth_ok && (out_rows & 3) == 0 && aligned_to(call->out_dev[f], out_align);
        if (s.ds_rep < 0 && depth_rows != w) s.ds_rep = f;
        if (s.final_rep < 0 && (depth_rows != w || out_rows != w)) s.final_rep = f;
    }
    s.ds_rep = std::max(s.ds_rep, 0);
    s.final_rep = std::max(s.final_rep, 0);
    s.ds_rows_per_lane = ds_tiles <= t.ds_small_max_tiles ? 1 : kMipRowsPerLane;
    s.render_tile_h = render_tiles <= t.render_small_max_tiles ? kRenTileHSmall : kRenTileH;
    s.final_tile_h = final_tiles <= t.final_small_max_tiles ? kUpsTileHSmall : ups_tile_h(true);
    s.blend1_tile_h = (c.ao_format == MEAO_AO_R8 || t.blend_tall_forced) && l1_tiles >= t.blend_tall_min_tiles ? kUpsTileHTall : ups_tile_h(false);
    s.l1_tiles = l1_tiles;
}

// Step 3.  A waiting composite rides in this call's render launch, or runs now as plain launches: the 68-sample render kernel
// carries nothing, and the per-frame render kernels neither; the carrying kernel takes RGBA16F batches only
// (meao_composite_enqueue_format).
int settle_composite(meao_ctx *ctx, Call *call)
{
    if (ctx->pending_comp.frames > 0 &&
        (ctx->cfg.sample_set == MEAO_SAMPLES_EXHAUSTIVE || call->per_frame || ctx->pending_comp_format != MEAO_COLOR_RGBA16F)) {
        const int rc = flush_pending_composite(ctx, call->stream);
        if (rc != MEAO_OK) return rc;
    }
    call->shape.carry_composite = ctx->pending_comp.frames > 0 && ctx->pending_comp_format == MEAO_COLOR_RGBA16F;    // the others were flushed above
    return MEAO_OK;
}

// Step 4.  The announced next batch: its pass rides in this call's last kernel where the fused form applies (f32 depth, 16-byte
// loads, a workgroup per carried tile), else it runs as a launch of its own behind it.  Either way the next call finds it done.
// `next`: the builder of the announced pass -- its plan has the announced frames' size, which need not be this call's
// (meao_prefetch_batch_sized); the rule is carried_in_last_kernel (meao_launch.hpp).
// (Inside the render launch instead -- CarriedMips in the texel loop, round 6 -- it costs the same 56-60 us per 16 4K frames:
// profiles/r06_ab_next_downsample_in_render_vs_final_vs_own_launch.jsonl, r06_scripts/r06_downsample_in_render.patch.)
void decide_announced_pass(meao_ctx *ctx, const ArgBuilder &args, const ArgBuilder &next, Call *call)
{
    Prefetch &pre = ctx->prefetch;
    if (pre.next.n == 0) return;
    const uint32_t gen = pre.generation_for_next();
    if (call->mixed()) { call->shape.next = 2; return; }      // the carrying kernel has one size: a mixed call never uses it
    const DownsampleArgs lean = next.downsample(pre.next.n, pre.next.depth, pre.next.depth_pitch, pre.other(), gen, true, false);
    call->shape.next = carried_in_last_kernel(args.upsample(0, true), args.hi_depth(), lean, call->n, ctx->tuning.next_ds_own_launch) ? 1 : 2;
}

// Step 6, per-frame half.  Frame f's blocks (and the announced batch's frame f for the carried pass) into the leased ring slot,
// one copy; *pf = the device table.
int build_frame_table(meao_ctx *ctx, const Call &call, const LaunchList &list, TableRing<FrameArgs, 8>::Lease *lease, const FrameArgs **pf)
{
    const Prefetch &pre = ctx->prefetch;
    const int rc = ctx->frame_ring.acquire(ctx, call.stream, lease);
    if (rc != MEAO_OK) return rc;
    FrameArgs *stage = lease->host();
    const int count = std::max(call.n, call.shape.next != 0 ? pre.next.n : 0);
    for (int f = 0; f < count; ++f) {
        const ArgBuilder fa = f < call.n ? call.frame_builder(ctx, f) : call.builder(ctx, &ctx->plan, &ctx->prm);
        const bool own_next = call.next_per_frame && f < pre.next.n;
        const ArgBuilder fb = call.builder(ctx, own_next ? &pre.next.plan[f] : Call::next_shared_plan(ctx), own_next ? &pre.next.prm[f] : &ctx->prm);
        build_call_args(fa, fb, call.shape, list, &stage[f]);
    }
    lease->arm();      // from here on every exit of this call hands the slot back guarded
    MEAO_HIP(ctx, hipMemcpyAsync(lease->device(), stage, sizeof(FrameArgs) * count, hipMemcpyHostToDevice, call.stream));
    *pf = lease->device();
    return MEAO_OK;
}

// Step 6, mixed half.  The shared blocks of a mixed call select each launch's kernel and give its grid, nothing else (no kernel
// reads them): the blocks of a frame that takes the call's kernel (CallShape::ds_rep / final_rep), with the largest frame's tile
// or block count as the grid -- never frame 0's, never the context's plan's.
void grid_blocks_of_table(const Call &call, const FrameArgs *table, FrameArgs *shared)
{
    *shared = table[0];
    shared->ds = table[call.launch.ds_rep].ds;
    shared->up[0] = table[call.launch.final_rep].up[0];
    shared->hi = table[call.launch.final_rep].hi;
    int32_t ds = 0, render = 0, render_hq = 0, up[4] = {0, 0, 0, 0};
    for (int f = 0; f < call.n; ++f) {
        const FrameArgs &t = table[f];
        ds = std::max(ds, t.ds.tiles_x * t.ds.tiles_y);
        render = std::max(render, t.render.blocks_per_frame);
        render_hq = std::max(render_hq, t.render_hq.blocks_per_frame);
        for (int hi = 0; hi < 4; ++hi) up[hi] = std::max(up[hi], t.up[hi].tiles_x * t.up[hi].tiles_y);
    }
    shared->ds.tiles_x = ds; shared->ds.tiles_y = 1;
    shared->render.blocks_per_frame = render;
    shared->render_hq.blocks_per_frame = render_hq;
    for (int hi = 0; hi < 4; ++hi) { shared->up[hi].tiles_x = up[hi]; shared->up[hi].tiles_y = 1; }
}

// Step 7.  Issues the list: `shared` holds the kernarg copies, pf (or null) the call's table of per-frame blocks.
int submit_launches(meao_ctx *ctx, const LaunchList &list, const FrameArgs &shared, const FrameArgs *pf, int n, hipStream_t stream)
{
    const int ao_format = ctx->cfg.ao_format;
    hipEvent_t *ev = ctx->profiler.cur;
    uint32_t ran = 0;
    auto P = [&](auto member) { return pf ? &(pf->*member) : nullptr; };
    auto PU = [&](int hi) { return pf ? &pf->up[hi] : nullptr; };
    for (int i = 0; i < list.n; ++i) {
        const Launch &L = list.v[i];
        TraceRange tr(ctx->tracer, L.range);
        // one launch = one profiling slot: events right before and after it on its stream
        const bool timed = ctx->profiler.bracket(L.slot);
        if (timed && ev) MEAO_HIP(ctx, hipEventRecord(ev[L.slot * 2], stream));
        switch (L.step) {
        case Step::Downsample:
            MEAO_HIP(ctx, launch_downsample(shared.ds, n, stream, P(&FrameArgs::ds)));
            break;
        case Step::Render:
            MEAO_HIP(ctx, launch_render(shared.render, ao_format, n, stream, P(&FrameArgs::render)));
            break;
        case Step::RenderWithComposite:
            // the composite of frames an earlier call produced streams under this (VALU-bound) kernel
            MEAO_HIP(ctx, launch_render_with_composite(shared.render, ctx->pending_comp, ao_format, n, stream));
            ctx->pending_comp.frames = 0;
            break;
        case Step::RenderHq:
            MEAO_HIP(ctx, launch_render_wide(shared.render_hq, ao_format, n, stream, P(&FrameArgs::render_hq)));
            break;
        case Step::Blend:
            MEAO_HIP(ctx, launch_upsample(shared.up[L.hi], nullptr, ao_format, n, stream, PU(L.hi)));
            break;
        case Step::BlendTwoLevel:
            MEAO_HIP(ctx, launch_upsample_two_level(shared.up[2], shared.up[3], ao_format, n, stream, PU(2), PU(3)));
            break;
        case Step::BlendThreeLevel:
            MEAO_HIP(ctx, launch_upsample_three_level(shared.up[1], shared.up[2], shared.up[3], ao_format, n, stream, PU(1), PU(2), PU(3)));
            break;
        case Step::Final:
            MEAO_HIP(ctx, launch_upsample(shared.up[0], &shared.hi, ao_format, n, stream, PU(0), P(&FrameArgs::hi)));
            break;
        case Step::FinalWithNextDownsample:
            MEAO_HIP(ctx, launch_upsample_final_with_downsample(shared.up[0], shared.hi, shared.next_ds, ao_format, n, stream, PU(0),
                                                                P(&FrameArgs::hi), P(&FrameArgs::next_ds)));
            break;
        case Step::DownsampleNext:
            MEAO_HIP(ctx, launch_downsample(shared.next_ds, ctx->prefetch.next.n, stream, P(&FrameArgs::next_ds)));
            break;
        }
        if (timed) {
            ran |= 1u << L.slot;
            if (ev) MEAO_HIP(ctx, hipEventRecord(ev[L.slot * 2 + 1], stream));
        }
    }
    ctx->profiler.end_call(ran);
    return MEAO_OK;
}

// Step 8, second half.  What the buffers built on demand need of this call (debug ids 1, 6-9, 17), as it used them.
void record_last_call(meao_ctx *ctx, const Call &call)
{
    const meao_config &c = ctx->cfg;
    LastCall &last = ctx->last;
    for (int f = 0; f < call.n; ++f) {
        LastCall::Frame &lf = last.frame[f];
        lf.out = call.out_dev[f];
        lf.depth = call.depth_dev[f];
        depth_decode_constants(c.depth_format, call.plan_of[f]->zbuffer_params, *call.prm_of[f], lf.zp);
        lf.reversed_z = call.prm_of[f]->reversed_z != 0;
        for (int k = 0; k < 4; ++k) lf.pad[k] = call.plan_of[f]->render[k].pad_value;
        lf.width = call.plan_of[f]->mip[0].w;
        lf.height = call.plan_of[f]->mip[0].h;
        lf.depth_pitch = call.depth_rows(f) == lf.width ? 0 : static_cast<uint64_t>(call.depth_rows(f)) * depth_elem(c.depth_format);
        lf.out_pitch = call.out_rows(f) == lf.width ? 0 : static_cast<uint64_t>(call.out_rows(f)) * ao_elem(c);
    }
    last.frames = call.n;
    last.mixed = call.mixed();
    last.stream = call.stream;
}

// The launch sequence of one batch of device frames.
int run_batch(meao_ctx *ctx, Call &call)
{
    Prefetch &pre = ctx->prefetch;
    resolve_constants(ctx, &call);
    ctx->profiler.begin_call();

    // A previous call may already have downsampled exactly these frames (meao_prefetch_batch): the ready set is consumed either way.
    call.shape = BatchShape{};
    call.shape.frames = call.n;
    // (a mixed call consumes it unmatched: a ready set holds frames of one size)
    call.shape.prefetched = !call.mixed() && pre.matches(call.n, call.depth_dev, call.stream, call.depth_pitch, call.exact != 0, call.prm_of,
                                                         ctx->cfg.depth_format, ctx->cfg.width, ctx->cfg.height);
    pre.begin_call(call.shape.prefetched);
    int rc = settle_composite(ctx, &call);
    if (rc != MEAO_OK) return rc;
    decide_call_shape(ctx, &call);

    const ArgBuilder args = call.builder(ctx, &ctx->plan, &ctx->prm);
    const ArgBuilder next = call.builder(ctx, Call::next_shared_plan(ctx), &ctx->prm);
    decide_announced_pass(ctx, args, next, &call);
    const LaunchList list = plan_launches(ctx->cfg, call.launch.l1_tiles, ctx->tuning, call.shape);

    FrameArgs shared{};
    if (!call.mixed()) build_call_args(args, next, call.shape, list, &shared);
    const FrameArgs *pf = nullptr;
    TableRing<FrameArgs, 8>::Lease lease;
    if (call.per_frame && (rc = build_frame_table(ctx, call, list, &lease, &pf)) != MEAO_OK) return rc;
    if (call.mixed()) grid_blocks_of_table(call, lease.host(), &shared);

    rc = submit_launches(ctx, list, shared, pf, call.n, call.stream);
    if (rc != MEAO_OK) return rc;

    if (call.shape.next != 0) pre.promote(call.stream, call.exact != 0, ctx->prm, ctx->cfg.width, ctx->cfg.height);
    record_last_call(ctx, call);
    return MEAO_OK;
}

// meao_prefetch_batch_params / _pitched / _sized: params[] checked where n is in range (an n out of range is refused by the announcement itself)
int fs_params_checked(meao_ctx *ctx, const char *fn, int32_t n, const meao_params *params)
{
    if (params && n >= 1 && n <= ctx->cfg.max_batch) return validate_frame_params(ctx, n, params, fn);
    return MEAO_OK;
}

int checked_prefetch(meao_ctx *ctx, const char *fn, const FrameSet &fs)
{
    const int rc = fs_params_checked(ctx, fn, fs.n, fs.params);
    return rc != MEAO_OK ? rc : prefetch_batch_internal(ctx, fs);
}

}  // namespace

int meao::validate_frame_params(meao_ctx *ctx, int32_t n, const meao_params *params, const char *what)
{
    for (int f = 0; f < n; ++f) {
        if (params[f].struct_size != sizeof(meao_params))
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(what) + ": params[" + std::to_string(f) + "]: struct_size mismatch (ABI)");
        if (!params_valid(params[f]))
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT,
                        std::string(what) + ": params[" + std::to_string(f) + "]: non-finite or degenerate parameter");
    }
    return MEAO_OK;
}

// The final pass forms row offsets with __umul24 (stride < 2^24 texels) and every offset into caller memory is a 32-bit byte
// offset (the frame's last texel ends at most 2^32 - 1 bytes after its origin).
int meao::pitch_texels(meao_ctx *ctx, uint64_t pitch, uint64_t elem, const char *what, int32_t *out)
{
    return pitch_texels_of(ctx, ctx->cfg.width, ctx->cfg.height, pitch, elem, what, out);
}

int meao::pitch_texels_of(meao_ctx *ctx, int32_t width, int32_t height, uint64_t pitch, uint64_t elem, const char *what, int32_t *out)
{
    const uint64_t w = static_cast<uint64_t>(width), h = static_cast<uint64_t>(height);
    if (pitch == 0) { *out = width; return MEAO_OK; }
    if (pitch < w * elem) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(what) + ": smaller than a row (width x element size)");
    if (pitch % elem != 0) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(what) + ": not a multiple of the element size");
    if (pitch / elem >= (1ull << 24)) return fail(ctx, MEAO_ERR_UNSUPPORTED, std::string(what) + ": 2^24 texels or more");
    if ((h - 1) * pitch + w * elem > 0xffffffffull)
        return fail(ctx, MEAO_ERR_UNSUPPORTED, std::string(what) + ": a frame spans more than 2^32 - 1 bytes");
    *out = static_cast<int32_t>(pitch / elem);
    return MEAO_OK;
}

void meao::drop_announcement(meao_ctx *ctx, bool ready_too)
{
    if (ctx) ctx->prefetch.withdraw(ready_too);
}

int meao::validate_execute_batch(meao_ctx *ctx, const FrameSet &fs, int32_t *depth_rows, int32_t *out_rows)
{
    if (!ctx || !fs.depth || !fs.out) return MEAO_ERR_INVALID_ARGUMENT;
    if (fs.n < 1 || fs.n > ctx->cfg.max_batch) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_execute_batch: n must be 1..max_batch");
    if ((fs.depth_loc != MEAO_MEM_HOST && fs.depth_loc != MEAO_MEM_DEVICE) || (fs.out_loc != MEAO_MEM_HOST && fs.out_loc != MEAO_MEM_DEVICE))
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_execute_batch: bad memory location");
    for (int f = 0; f < fs.n; ++f)
        if (!fs.depth[f] || !fs.out[f]) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_execute_batch: null frame pointer");
    if (!ctx->arena) return fail(ctx, MEAO_ERR_OUT_OF_MEMORY, "meao_execute_batch: the context has no intermediates");
    if (fs.params) {
        const int vr = validate_frame_params(ctx, fs.n, fs.params, "meao_execute_batch_params");
        if (vr != MEAO_OK) return vr;
    }
    int vr = pitch_texels(ctx, fs.depth_pitch, depth_elem(ctx->cfg.depth_format), "meao_execute_batch_pitched: depth_pitch", depth_rows);
    if (vr == MEAO_OK) vr = pitch_texels(ctx, fs.out_pitch, ao_elem(ctx->cfg), "meao_execute_batch_pitched: ao_pitch", out_rows);
    return vr;
}

int meao::validate_execute_batch_extents(meao_ctx *ctx, const FrameSet &fs, int32_t *depth_rows, int32_t *out_rows, bool *uniform)
{
    static const char fn[] = "meao_execute_batch_extents";
    if (!ctx || !fs.depth || !fs.out || !fs.extents) return MEAO_ERR_INVALID_ARGUMENT;
    if (fs.n < 1 || fs.n > ctx->cfg.max_batch) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": n must be 1..max_batch");
    if (fs.depth_loc != MEAO_MEM_DEVICE || fs.out_loc != MEAO_MEM_DEVICE)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": DEVICE surfaces only");
    for (int f = 0; f < fs.n; ++f)
        if (!fs.depth[f] || !fs.out[f])
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": frame " + std::to_string(f) + ": null frame pointer");
    if (!ctx->arena) return fail(ctx, MEAO_ERR_OUT_OF_MEMORY, std::string(fn) + ": the context has no intermediates");
    if (fs.params) {
        const int vr = validate_frame_params(ctx, fs.n, fs.params, fn);
        if (vr != MEAO_OK) return vr;
    }
    *uniform = true;
    for (int f = 0; f < fs.n; ++f) {
        const meao_extent &e = fs.extents[f];
        const std::string at = std::string(fn) + ": extents[" + std::to_string(f) + "]";
        if (!size_valid(e.width, e.height)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, at + ".width/height out of range [1, 32768]");
        if (!ctx->within_capacity(e.width, e.height))
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, at + ".width/height: not inside the context's capacity (its reservation, else its size)");
        int vr = pitch_texels_of(ctx, e.width, e.height, e.depth_pitch, depth_elem(ctx->cfg.depth_format), (at + ".depth_pitch").c_str(), &depth_rows[f]);
        if (vr == MEAO_OK) vr = pitch_texels_of(ctx, e.width, e.height, e.ao_pitch, ao_elem(ctx->cfg), (at + ".ao_pitch").c_str(), &out_rows[f]);
        if (vr != MEAO_OK) return vr;
        *uniform = *uniform && e.width == ctx->cfg.width && e.height == ctx->cfg.height && depth_rows[f] == depth_rows[0] && out_rows[f] == out_rows[0];
    }
    return MEAO_OK;
}

namespace {

// meao_execute_batch_extents, validated: the mixed call
int execute_mixed_batch(meao_ctx *ctx, const FrameSet &fs, const int32_t *depth_rows, const int32_t *out_rows, meao_stream stream_)
{
    const int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    Call call;
    call.n = fs.n; call.depth_dev = fs.depth; call.out_dev = fs.out; call.fp = fs.params;
    call.stream = stream_ ? static_cast<hipStream_t>(stream_) : ctx->own_stream;
    call.depth_pitch = call.out_pitch = ctx->cfg.width;     // (of the blocks no launch of a mixed call reads)
    call.extents = fs.extents; call.depth_pitch_of = depth_rows; call.out_pitch_of = out_rows;
    return run_batch(ctx, call);
}

}  // namespace

int meao::execute_batch_internal(meao_ctx *ctx, const FrameSet &fs, meao_stream stream_, bool wait_for_host)
{
    if (fs.extents) {
        int32_t rows_d[MEAO_MAX_BATCH], rows_o[MEAO_MAX_BATCH];
        bool uniform = false;
        const int vr = validate_execute_batch_extents(ctx, fs, rows_d, rows_o, &uniform);
        if (vr != MEAO_OK) return vr;
        if (!uniform) return execute_mixed_batch(ctx, fs, rows_d, rows_o, stream_);
        FrameSet same = fs;       // every frame at the context's size with one pair of pitches: meao_execute_batch_pitched
        same.extents = nullptr; same.depth_pitch = fs.extents[0].depth_pitch; same.out_pitch = fs.extents[0].ao_pitch;
        return execute_batch_internal(ctx, same, stream_, wait_for_host);
    }
    int32_t depth_rows = 0, out_rows = 0;     // row strides in texels
    {
        const int vr = validate_execute_batch(ctx, fs, &depth_rows, &out_rows);
        if (vr != MEAO_OK) return vr;
    }
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    hipStream_t stream = stream_ ? static_cast<hipStream_t>(stream_) : ctx->own_stream;

    const meao_config &c = ctx->cfg;
    const int n = fs.n;
    const uint64_t depth_row = static_cast<uint64_t>(c.width) * depth_elem(c.depth_format), out_row = static_cast<uint64_t>(c.width) * ao_elem(c);
    const uint64_t depth_bytes = depth_row * c.height, out_bytes = out_row * c.height;
    const bool depth_packed = depth_rows == c.width, out_packed = out_rows == c.width;
    const void *depth_dev[MEAO_MAX_BATCH];
    void *out_dev[MEAO_MAX_BATCH];
    if (fs.depth_loc == MEAO_MEM_HOST) {      // staged packed, one aligned frame after the other
        const uint64_t frame = align_up(depth_bytes);
        rc = ctx->stage_depth.reserve(ctx, frame * c.max_batch, "hipMalloc (depth staging)");
        if (rc != MEAO_OK) return rc;
        for (int f = 0; f < n; ++f) {
            char *d = ctx->stage_depth.ptr + frame * f;
            if (depth_packed) MEAO_HIP(ctx, hipMemcpyAsync(d, fs.depth[f], depth_bytes, hipMemcpyHostToDevice, stream));
            else MEAO_HIP(ctx, hipMemcpy2DAsync(d, depth_row, fs.depth[f], fs.depth_pitch, depth_row, c.height, hipMemcpyHostToDevice, stream));
            depth_dev[f] = d;
        }
        depth_rows = c.width;
    } else {
        for (int f = 0; f < n; ++f) depth_dev[f] = fs.depth[f];
    }
    if (fs.out_loc == MEAO_MEM_HOST) {
        const uint64_t frame = align_up(out_bytes);
        rc = ctx->stage_out.reserve(ctx, frame * c.max_batch, "hipMalloc (result staging)");
        if (rc != MEAO_OK) return rc;
        for (int f = 0; f < n; ++f) out_dev[f] = ctx->stage_out.ptr + frame * f;
        out_rows = c.width;
    } else {
        for (int f = 0; f < n; ++f) out_dev[f] = fs.out[f];
    }

    Call call;
    call.n = n; call.depth_dev = depth_dev; call.out_dev = out_dev; call.stream = stream; call.fp = fs.params;
    call.depth_pitch = depth_rows; call.out_pitch = out_rows;
    rc = run_batch(ctx, call);
    if (rc != MEAO_OK) return rc;

    if (fs.out_loc == MEAO_MEM_HOST)
        for (int f = 0; f < n; ++f) {
            if (out_packed) MEAO_HIP(ctx, hipMemcpyAsync(fs.out[f], out_dev[f], out_bytes, hipMemcpyDeviceToHost, stream));
            else MEAO_HIP(ctx, hipMemcpy2DAsync(fs.out[f], fs.out_pitch, out_dev[f], out_row, out_row, c.height, hipMemcpyDeviceToHost, stream));
        }
    if (wait_for_host && (fs.out_loc == MEAO_MEM_HOST || fs.depth_loc == MEAO_MEM_HOST)) {
        note_sync(ctx);
        MEAO_HIP(ctx, hipStreamSynchronize(stream));
    }
    return MEAO_OK;
}

int meao::prefetch_batch_internal(meao_ctx *ctx, const FrameSet &fs, int32_t width, int32_t height)
{
    if (!ctx || !fs.depth) return MEAO_ERR_INVALID_ARGUMENT;
    const bool sized = (width != 0 || height != 0) && !(width == ctx->cfg.width && height == ctx->cfg.height);
    if (sized && !(width >= 1 && height >= 1 && ctx->within_reservation(width, height)))
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_prefetch_batch_sized: width/height: not inside the context's reservation (meao_reserve)");
    if (!sized) { width = ctx->cfg.width; height = ctx->cfg.height; }
    if (fs.n < 1 || fs.n > ctx->cfg.max_batch) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_prefetch_batch: n must be 1..max_batch");
    for (int f = 0; f < fs.n; ++f)
        if (!fs.depth[f]) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_prefetch_batch: null frame pointer");
    int32_t rows = 0;
    int rc = pitch_texels_of(ctx, width, height, fs.depth_pitch, depth_elem(ctx->cfg.depth_format),
                             sized ? "meao_prefetch_batch_sized: depth_pitch" : "meao_prefetch_batch_pitched: depth_pitch", &rows);
    if (rc != MEAO_OK) return rc;
    rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    if (!ctx->two_ds_sets) {
        // Created without cfg.pipelined: the first announcement re-lays the slots out with a second
        // downsample set (device-wide synchronisation + allocation, once).  On failure the context is unchanged.
        note_sync(ctx);
        MEAO_HIP(ctx, hipDeviceSynchronize());
        rc = reallocate(ctx, ctx->cfg, true, ctx->cap_w, ctx->cap_h);
        if (rc != MEAO_OK) return rc;
    }
    ctx->prefetch.announce(ctx->cfg, width, height, sized, ctx->prm, fs.n, fs.depth, rows, fs.params);
    return MEAO_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" {

int32_t meao_execute_batch(meao_ctx *ctx, int32_t n, const void *const *depth, int32_t depth_loc,
                           void *const *ao_out, int32_t out_loc, meao_stream stream_)
{
    return execute_batch_internal(ctx, FrameSet{n, depth, 0, depth_loc, ao_out, 0, out_loc, nullptr}, stream_, true);
}

int32_t meao_execute_batch_params(meao_ctx *ctx, int32_t n, const void *const *depth, int32_t depth_loc, void *const *ao_out,
                                  int32_t out_loc, const meao_params *params, meao_stream stream_)
{
    if (!params) return ctx ? fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_execute_batch_params: params is null") : MEAO_ERR_INVALID_ARGUMENT;
    return execute_batch_internal(ctx, FrameSet{n, depth, 0, depth_loc, ao_out, 0, out_loc, params}, stream_, true);
}

int32_t meao_execute_batch_pitched(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch, int32_t depth_loc,
                                   void *const *ao_out, uint64_t ao_pitch, int32_t out_loc, const meao_params *params, meao_stream stream_)
{
    return execute_batch_internal(ctx, FrameSet{n, depth, depth_pitch, depth_loc, ao_out, ao_pitch, out_loc, params}, stream_, true);
}

int32_t meao_execute_batch_extents(meao_ctx *ctx, int32_t n, const void *const *depth, void *const *ao_out, const meao_extent *extents,
                                   const meao_params *params, meao_stream stream_)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    if (!depth || !ao_out || !extents) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_execute_batch_extents: depth, ao_out or extents is null");
    FrameSet fs{n, depth, 0, MEAO_MEM_DEVICE, ao_out, 0, MEAO_MEM_DEVICE, params};
    fs.extents = extents;
    return execute_batch_internal(ctx, fs, stream_, true);
}

int32_t meao_execute(meao_ctx *ctx, const void *depth, int32_t depth_loc, void *ao_out, int32_t out_loc,
                     meao_stream stream)
{
    const void *d[1] = {depth};
    void *o[1] = {ao_out};
    return meao_execute_batch(ctx, 1, d, depth_loc, o, out_loc, stream);
}

int32_t meao_prefetch_batch(meao_ctx *ctx, int32_t n, const void *const *depth)
{
    return prefetch_batch_internal(ctx, FrameSet{n, depth, 0, MEAO_MEM_DEVICE, nullptr, 0, MEAO_MEM_DEVICE, nullptr});
}

int32_t meao_prefetch_batch_params(meao_ctx *ctx, int32_t n, const void *const *depth, const meao_params *params)
{
    if (!ctx || !params) return MEAO_ERR_INVALID_ARGUMENT;
    return checked_prefetch(ctx, "meao_prefetch_batch_params", FrameSet{n, depth, 0, MEAO_MEM_DEVICE, nullptr, 0, MEAO_MEM_DEVICE, params});
}

int32_t meao_prefetch_batch_pitched(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch, const meao_params *params)
{
    if (!ctx || !depth) return MEAO_ERR_INVALID_ARGUMENT;
    return checked_prefetch(ctx, "meao_prefetch_batch_pitched", FrameSet{n, depth, depth_pitch, MEAO_MEM_DEVICE, nullptr, 0, MEAO_MEM_DEVICE, params});
}

int32_t meao_prefetch_batch_sized(meao_ctx *ctx, int32_t width, int32_t height, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                  const meao_params *params)
{
    if (!ctx || !depth) return MEAO_ERR_INVALID_ARGUMENT;
    if (width < 1 || height < 1) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_prefetch_batch_sized: width/height must be at least 1");
    const int rc = fs_params_checked(ctx, "meao_prefetch_batch_sized", n, params);
    if (rc != MEAO_OK) return rc;
    return prefetch_batch_internal(ctx, FrameSet{n, depth, depth_pitch, MEAO_MEM_DEVICE, nullptr, 0, MEAO_MEM_DEVICE, params}, width, height);
}

}  // extern "C"
