// meao_debug.cpp -- the intermediates of the last execute (meao_get_intermediate) and their debug view (meao_debug_view).
#include <hip/hip_runtime.h>

#include "meao_ctx.hpp"

using namespace meao;

namespace {

// A pitched device frame of the last call (debug ids 1 and 17) packed into the context's scratch first (not a hot path);
// *frame = the packed copy.
int pack_last_frame(meao_ctx *ctx, const LastCall::Frame &last, const void **frame, uint64_t pitch, uint64_t elem, hipStream_t s)
{
    const uint64_t row = static_cast<uint64_t>(last.width) * elem;
    const int rc = ctx->pack_scratch.reserve(ctx, row * last.height, "hipMalloc (packed copy of a pitched frame)");
    if (rc != MEAO_OK) return rc;
    MEAO_HIP(ctx, hipMemcpy2DAsync(ctx->pack_scratch.ptr, row, *frame, pitch, row, last.height, hipMemcpyDeviceToDevice, s));
    *frame = ctx->pack_scratch.ptr;
    return MEAO_OK;
}

// Device address of debug buffer `debug_id` of batch slot `frame` (LinearDepth and TiledDepth are built on demand, in the
// scratch for the buffers the hot path never materialises).
int locate_debug_buffer(meao_ctx *ctx, int32_t frame, int32_t debug_id, const meao_desc &d, hipStream_t s, const void **out_src)
{
    const SlotLayout &lay = ctx->lay;
    const LastCall::Frame &last = ctx->last.frame[frame];
    const char *slot = ctx->arena + lay.slot_bytes * frame;
    const int nl = ctx->cfg.num_levels, ds_cur = ctx->prefetch.ds_cur;
    if (debug_id == 1) {
        // LinearDepth: materialised on demand from the raw depth frame of the last call (its one consumer on the hot path,
        // the full-resolution upsample, evaluates Linearize itself).  The caller's depth frame must still be alive.
        int rc = ctx->atlas_scratch.reserve(ctx, d.bytes, "hipMalloc (debug scratch)");
        if (rc != MEAO_OK) return rc;
        LinearDepthArgs la{};
        la.depth = last.depth;
        if (last.depth_pitch != 0) {
            rc = pack_last_frame(ctx, last, &la.depth, last.depth_pitch, depth_elem(ctx->cfg.depth_format), s);
            if (rc != MEAO_OK) return rc;
        }
        la.dst = reinterpret_cast<uint16_t *>(ctx->atlas_scratch.ptr);
        la.pixels = static_cast<int64_t>(d.width) * d.height;
        la.depth_format = ctx->cfg.depth_format;
        la.reversed_z = last.reversed_z;          // the parameters the last call used for this frame
        la.f16_rtne = ctx->cfg.f16_rounding == MEAO_F16_RTNE;
        la.zp0 = last.zp[0];
        la.zp1 = last.zp[1];
        MEAO_HIP(ctx, launch_linear_depth(la, s));
        *out_src = ctx->atlas_scratch.ptr;
    } else if (debug_id <= 5) *out_src = slot + lay.off_low_of(ds_cur, debug_id - 2);
    else if (debug_id <= 9) {
        // TiledDepth<level>: materialised on demand from LowDepth<level> (the hot path samples
        // LowDepth directly and never builds the de-interleaved arrays).
        const int level = debug_id - 5;
        const int rc = ctx->atlas_scratch.reserve(ctx, d.bytes, "hipMalloc (debug scratch)");
        if (rc != MEAO_OK) return rc;
        TileAtlasArgs ta{};
        ta.src = reinterpret_cast<const float *>(slot + lay.off_low_of(ds_cur, level - 1));
        ta.dst = reinterpret_cast<uint16_t *>(ctx->atlas_scratch.ptr);
        const Dims lv = level_dims(last.width, last.height, level);     // (the frame's own size after a mixed call)
        ta.lw = lv.w; ta.lh = lv.h;
        ta.sw = d.width; ta.sh = d.height;
        ta.pad_value = last.pad[level - 1];
        ta.f16_rtne = ctx->cfg.f16_rounding == MEAO_F16_RTNE;
        MEAO_HIP(ctx, launch_tile_atlas(ta, s));
        *out_src = ctx->atlas_scratch.ptr;
    } else if (debug_id <= 13) {
        if (debug_id - 9 > nl) return fail(ctx, MEAO_ERR_UNSUPPORTED, "debug buffer: level not rendered (num_levels)");
        *out_src = slot + lay.off_occ[debug_id - 10];
    } else if (debug_id <= 16) {
        if (debug_id - 13 > nl - 1) return fail(ctx, MEAO_ERR_UNSUPPORTED, "debug buffer: level not combined (num_levels)");
        *out_src = slot + lay.off_comb[debug_id - 14];
    } else if (debug_id == 17) {
        *out_src = last.out;
        if (last.out_pitch != 0) return pack_last_frame(ctx, last, out_src, last.out_pitch, ao_elem(ctx->cfg), s);
    } else {
        const int level = debug_id - MEAO_DEBUG_OCCLUSION_HQ1 + 1;
        if (!level_has_hq(nl, ctx->cfg.hq_levels, level))
            return fail(ctx, MEAO_ERR_UNSUPPORTED, "debug buffer: this level has no Render.main pass (hq_levels)");
        *out_src = slot + lay.off_hq[level - 1];
    }
    return MEAO_OK;
}

}  // namespace

extern "C" {

int32_t meao_get_intermediate(meao_ctx *ctx, int32_t frame, int32_t debug_id, void *dst, uint64_t dst_capacity,
                              int32_t dst_loc, meao_desc *out_desc)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    meao_desc d{};
    if (!describe_buffer(ctx->cfg.width, ctx->cfg.height, ctx->cfg.ao_format, debug_id, &d))
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_get_intermediate: debug_id must be 1..21");
    if (out_desc) *out_desc = d;
    if (!dst) return MEAO_OK;
    if (!ctx->arena) return fail(ctx, MEAO_ERR_OUT_OF_MEMORY, "meao_get_intermediate: the context has no intermediates");
    if (frame < 0 || frame >= ctx->last.frames)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_get_intermediate: frame not produced by the last execute");
    if (ctx->last.mixed) {      // the buffers of a mixed call's frame have that frame's size
        describe_buffer(ctx->last.frame[frame].width, ctx->last.frame[frame].height, ctx->cfg.ao_format, debug_id, &d);
        if (out_desc) *out_desc = d;
    }
    if (dst_capacity < d.bytes) return fail(ctx, MEAO_ERR_BUFFER_TOO_SMALL, "meao_get_intermediate: dst_capacity < desc.bytes");
    if (dst_loc != MEAO_MEM_HOST && dst_loc != MEAO_MEM_DEVICE) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    hipStream_t s = ctx->last.stream;
    const void *src = nullptr;
    rc = locate_debug_buffer(ctx, frame, debug_id, d, s, &src);
    if (rc != MEAO_OK) return rc;
    MEAO_HIP(ctx, hipMemcpyAsync(dst, src, d.bytes,
                                 dst_loc == MEAO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    note_sync(ctx);
    MEAO_HIP(ctx, hipStreamSynchronize(s));
    return MEAO_OK;
}

int32_t meao_debug_view(meao_ctx *ctx, int32_t frame, int32_t debug_id, void *out, int32_t out_loc, meao_stream stream_)
{
    if (!ctx || !out) return MEAO_ERR_INVALID_ARGUMENT;
    meao_desc d{};
    if (!describe_buffer(ctx->cfg.width, ctx->cfg.height, ctx->cfg.ao_format, debug_id, &d))
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_debug_view: debug_id must be 1..21");
    if (!ctx->arena) return fail(ctx, MEAO_ERR_OUT_OF_MEMORY, "meao_debug_view: the context has no intermediates");
    if (frame < 0 || frame >= ctx->last.frames)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_debug_view: frame not produced by the last execute");
    // (after a mixed call: the frame's own size, for the buffer and for the view)
    const int32_t view_w = ctx->last.mixed ? ctx->last.frame[frame].width : ctx->cfg.width;
    const int32_t view_h = ctx->last.mixed ? ctx->last.frame[frame].height : ctx->cfg.height;
    if (ctx->last.mixed) describe_buffer(view_w, view_h, ctx->cfg.ao_format, debug_id, &d);
    if (out_loc != MEAO_MEM_HOST && out_loc != MEAO_MEM_DEVICE) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    hipStream_t s = stream_ ? static_cast<hipStream_t>(stream_) : ctx->last.stream;
    const void *src = nullptr;
    rc = locate_debug_buffer(ctx, frame, debug_id, d, s, &src);
    if (rc != MEAO_OK) return rc;
    const uint64_t out_bytes = static_cast<uint64_t>(view_w) * view_h * ao_elem(ctx->cfg);
    void *dev_out = out;
    if (out_loc == MEAO_MEM_HOST) {   // own staging buffer: stage_out may hold the results (debug id 17)
        rc = ctx->stage_view.reserve(ctx, align_up(out_bytes), "hipMalloc (debug view staging)");
        if (rc != MEAO_OK) return rc;
        dev_out = ctx->stage_view.ptr;
    }
    DebugViewArgs dv{};
    dv.src = src; dv.dst = dev_out;
    dv.sw = d.width; dv.sh = d.height; dv.slices = d.slices; dv.src_format = d.format;
    dv.w = view_w; dv.h = view_h;
    dv.f16_rtne = ctx->cfg.f16_rounding == MEAO_F16_RTNE;
    MEAO_HIP(ctx, launch_debug_view(dv, ctx->cfg.ao_format, s));
    if (out_loc == MEAO_MEM_HOST) {
        MEAO_HIP(ctx, hipMemcpyAsync(out, dev_out, out_bytes, hipMemcpyDeviceToHost, s));
        note_sync(ctx);
        MEAO_HIP(ctx, hipStreamSynchronize(s));
    }
    return MEAO_OK;
}

}  // extern "C"
