// meao_composite.cpp -- the composite calls of the C ABI (meao_composite*, meao_execute_batch_shaded): one frame now, a batch
// waiting for the next execute's render launch, or a batch in one launch of its own.
#include <hip/hip_runtime.h>

#include <string>

#include "meao_ctx.hpp"

using namespace meao;

namespace {

// Bytes per texel of a meao_color_format, 0 = not one; the texels of it that a lane of the vector form takes (16 bytes of colour).
uint64_t color_elem(int32_t color_format)
{
    switch (color_format) {
    case MEAO_COLOR_RGBA16F: return 8;
    case MEAO_COLOR_RGBA32F: return 16;
    case MEAO_COLOR_RGBA8: case MEAO_COLOR_R11G11B10F: case MEAO_COLOR_RGBA8_SRGB: return 4;
    default: return 0;
    }
}
uint32_t color_lane_texels(int32_t color_format) { return static_cast<uint32_t>(16 / color_elem(color_format)); }

// The pitches of meao_composite*_pitched (bytes, 0 = tightly packed) -> CompositePitches; `fn` names the entry point in the error.
// on = 0 where every surface is tightly packed: exactly the packed kernels' path.
int composite_pitches(meao_ctx *ctx, const char *fn, const CompositeTargets &t, CompositePitches *out)
{
    const bool has_gbuffer0 = t.gbuffer0 != nullptr;
    const uint64_t celem = color_elem(t.color_format);
    if (celem == 0) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": color_format: not a meao_color_format");
    int32_t ao_row = ctx->cfg.width, color_row = ctx->cfg.width, g_row = ctx->cfg.width;
    if (t.ao_pitch != 0 || t.color_pitch != 0 || (t.gbuffer0_pitch != 0 && has_gbuffer0)) {       // packed calls have nothing to check
        // the argument's name is built only where a pitch is given (0 cannot fail)
        const auto texels = [&](uint64_t pitch, uint64_t elem, const char *which, int32_t *row) {
            return pitch_texels(ctx, pitch, elem, pitch ? (std::string(fn) + ": " + which).c_str() : "", row);
        };
        int rc = texels(t.ao_pitch, ao_elem(ctx->cfg), "ao_pitch", &ao_row);
        if (rc == MEAO_OK) rc = texels(t.color_pitch, celem, "color_pitch", &color_row);
        if (rc == MEAO_OK && has_gbuffer0) rc = texels(t.gbuffer0_pitch, 4, "gbuffer0_pitch", &g_row);
        if (rc != MEAO_OK) return rc;
    }
    *out = CompositePitches{};
    out->ao = static_cast<uint32_t>(ao_row); out->color = static_cast<uint32_t>(color_row); out->gbuffer0 = static_cast<uint32_t>(g_row);
    out->w = ctx->cfg.width; out->h = ctx->cfg.height;
    out->on = ao_row != ctx->cfg.width || color_row != ctx->cfg.width || g_row != ctx->cfg.width;
    out->vec = (color_row & 1) == 0 && (ao_row & 1) == 0;      // colour rows 16 bytes apart, AO rows two texels apart; the bases: composite_vec_base
    if (t.color_format != MEAO_COLOR_RGBA16F) {
        // a packed frame is one row of width x height texels to the kernel, with 32-bit byte offsets like any row
        if (static_cast<uint64_t>(ctx->cfg.width) * ctx->cfg.height * celem > 0xffffffffull)
            return fail(ctx, MEAO_ERR_UNSUPPORTED, std::string(fn) + ": color: a frame spans more than 2^32 - 1 bytes");
        // rows of whole 16-byte colour accesses, each with its AO texels in one aligned load (nothing to ask of a packed frame's rows)
        out->vec = !out->on || (static_cast<uint64_t>(color_row) * celem % 16 == 0 && static_cast<uint32_t>(ao_row) % color_lane_texels(t.color_format) == 0);
    }
    return MEAO_OK;
}

// The vector form's conditions on a frame's bases: colour a multiple of 16 bytes, AO a multiple of the AO texels of a lane (two for RGBA16F).
bool composite_vec_base(const meao_ctx *ctx, const void *ao, const void *color, int32_t color_format)
{
    return aligned_to(color, 16) && aligned_to(ao, color_lane_texels(color_format) * ao_elem(ctx->cfg));
}

// meao_composite*: the one frame of `t` (n = 1) now, on the given stream; loc = where its surfaces live.
int composite_one(meao_ctx *ctx, const char *fn, const CompositeTargets &t, int32_t loc, meao_stream stream_)
{
    const void *ao = t.ao[0];
    void *color = t.color[0], *gbuffer0 = t.gbuffer0 ? t.gbuffer0[0] : nullptr;
    if (!ctx || !ao || !color) return MEAO_ERR_INVALID_ARGUMENT;
    if (t.mode < MEAO_COMPOSITE_MULTIPLY || t.mode > MEAO_COMPOSITE_DEBUG) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": unknown mode");
    if (t.mode == MEAO_COMPOSITE_AMBIENT_ONLY && !gbuffer0)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": AMBIENT_ONLY needs the GBuffer0 target");
    if (loc != MEAO_MEM_HOST && loc != MEAO_MEM_DEVICE) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": bad memory location");
    CompositePitches pitch{};
    int rc = composite_pitches(ctx, fn, t, &pitch);
    if (rc != MEAO_OK) return rc;
    rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    hipStream_t stream = stream_ ? static_cast<hipStream_t>(stream_) : ctx->own_stream;
    const uint64_t px = static_cast<uint64_t>(ctx->cfg.width) * ctx->cfg.height;
    const uint64_t celem = color_elem(t.color_format);
    const uint64_t ao_bytes = px * ao_elem(ctx->cfg), color_bytes = px * celem, g_bytes = px * 4;
    CompositeArgs ca{};
    ca.pixels = static_cast<int64_t>(px);
    ca.mode = t.mode;
    ca.color_format = t.color_format;
    char *scratch = nullptr;
    if (loc == MEAO_MEM_HOST) {     // tools / tests: stage through one temporary device buffer (packed there, whatever the host pitches)
        const uint64_t h = static_cast<uint64_t>(ctx->cfg.height);
        const uint64_t ao_row = ao_bytes / h, color_row = color_bytes / h, g_row = g_bytes / h;
        const uint64_t ao_src = uint64_t(pitch.ao) * ao_elem(ctx->cfg), color_src = uint64_t(pitch.color) * celem, g_src = uint64_t(pitch.gbuffer0) * 4;
        MEAO_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&scratch), align_up(ao_bytes) + align_up(color_bytes) + g_bytes));
        char *d_ao = scratch, *d_color = scratch + align_up(ao_bytes), *d_g = d_color + align_up(color_bytes);
        auto copy = [&](void *dst, uint64_t dst_pitch, const void *src, uint64_t src_pitch, uint64_t row, hipMemcpyKind kind) {
            if (dst_pitch == row && src_pitch == row) return hipMemcpyAsync(dst, src, row * h, kind, stream);      // packed: one copy, as ever
            return hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, row, h, kind, stream);
        };
        hipError_t e = copy(d_ao, ao_row, ao, ao_src, ao_row, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = copy(d_color, color_row, color, color_src, color_row, hipMemcpyHostToDevice);
        if (e == hipSuccess && gbuffer0) e = copy(d_g, g_row, gbuffer0, g_src, g_row, hipMemcpyHostToDevice);
        ca.ao = d_ao; ca.color = d_color; ca.gbuffer0 = gbuffer0 ? d_g : nullptr;
        ca.pitch.vec = 1;       // packed at aligned bases (read by the colour formats other than RGBA16F only)
        if (e == hipSuccess) e = launch_composite(ca, ctx->cfg.ao_format, stream);
        if (e == hipSuccess) e = copy(color, color_src, d_color, color_row, color_row, hipMemcpyDeviceToHost);
        if (e == hipSuccess && gbuffer0) e = copy(gbuffer0, g_src, d_g, g_row, g_row, hipMemcpyDeviceToHost);
        note_sync(ctx);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        (void)hipFree(scratch);
        if (e != hipSuccess) return fail_hip(ctx, e, (std::string(fn) + " (host staging)").c_str());
        return MEAO_OK;
    }
    ca.ao = ao; ca.color = color; ca.gbuffer0 = gbuffer0;
    ca.pitch = pitch;
    ca.pitch.vec = pitch.vec && composite_vec_base(ctx, ao, color, t.color_format);
    MEAO_HIP(ctx, launch_composite(ca, ctx->cfg.ao_format, stream));
    return MEAO_OK;
}

// The single-frame entry points: one frame as a CompositeTargets of n = 1.
int composite_single(meao_ctx *ctx, const char *fn, int32_t mode, const void *ao, uint64_t ao_pitch, void *color, int32_t color_format,
                     uint64_t color_pitch, void *gbuffer0, uint64_t gbuffer0_pitch, int32_t loc, meao_stream stream)
{
    return composite_one(ctx, fn, CompositeTargets{mode, 1, &ao, ao_pitch, &color, color_format, color_pitch, gbuffer0 ? &gbuffer0 : nullptr, gbuffer0_pitch},
                         loc, stream);
}

// The checks of meao_composite_enqueue_format under the name `fn`, the pitches on success.  Touches nothing.
int composite_enqueue_validate(meao_ctx *ctx, const char *fn, const CompositeTargets &t, CompositePitches *pitch)
{
    if (!ctx || !t.ao || !t.color) return MEAO_ERR_INVALID_ARGUMENT;
    if (t.mode < MEAO_COMPOSITE_MULTIPLY || t.mode > MEAO_COMPOSITE_DEBUG) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": unknown mode");
    if (t.n < 1 || t.n > MEAO_MAX_BATCH) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": n must be 1..MEAO_MAX_BATCH");
    if (t.mode == MEAO_COMPOSITE_AMBIENT_ONLY && !t.gbuffer0)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": AMBIENT_ONLY needs the GBuffer0 targets");
    for (int f = 0; f < t.n; ++f)
        if (!t.ao[f] || !t.color[f] || (t.mode == MEAO_COMPOSITE_AMBIENT_ONLY && !t.gbuffer0[f]))
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": null frame pointer");
    return composite_pitches(ctx, fn, t, pitch);
}

// The checks of a batched composite under the name `fn`: n against the context's max_batch (the tables' size), then those of
// meao_composite_enqueue_format.  Touches nothing.
int composite_batch_validate(meao_ctx *ctx, const char *fn, const CompositeTargets &t, CompositePitches *pitch)
{
    if (!ctx || !t.ao || !t.color) return MEAO_ERR_INVALID_ARGUMENT;
    if (t.n < 1 || t.n > ctx->cfg.max_batch) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": n must be 1..max_batch");
    return composite_enqueue_validate(ctx, fn, t, pitch);
}

// The batched composite: frames 0 .. n-1 in ONE composite_kernel launch on `stream` (every argument already validated).  Their
// origins go through a slot of the context's table ring; one form (vector or per-texel) for the whole batch, as for an enqueued one.
int composite_batch_launch(meao_ctx *ctx, const CompositeTargets &t, CompositePitches pitch, hipStream_t stream)
{
    TableRing<CompositeFrame, 8>::Lease lease;
    const int rc = ctx->comp_ring.acquire(ctx, stream, &lease);
    if (rc != MEAO_OK) return rc;
    CompositeFrame *stage = lease.host();
    for (int f = 0; f < t.n; ++f) {
        stage[f] = CompositeFrame{t.ao[f], t.color[f], t.gbuffer0 ? t.gbuffer0[f] : nullptr};
        pitch.vec = pitch.vec && composite_vec_base(ctx, t.ao[f], t.color[f], t.color_format);
    }
    CompositeArgs ca{};
    ca.pixels = static_cast<int64_t>(ctx->cfg.width) * ctx->cfg.height;
    ca.mode = t.mode;
    ca.pitch = pitch;
    ca.color_format = t.color_format;
    ca.frames = lease.device();
    lease.arm();       // the slot is handed back guarded whatever happens from here: the copy may be in flight
    hipError_t e = hipMemcpyAsync(lease.device(), stage, sizeof(CompositeFrame) * t.n, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_composite(ca, ctx->cfg.ao_format, stream, t.n);
    if (e != hipSuccess) return fail_hip(ctx, e, "composite_batch_launch");
    return MEAO_OK;
}

// composite_pitches / composite_vec_base for one frame of its own size (meao_composite_batch_extents): e's three pitches against
// e's width and height instead of ctx->cfg, into entry `out` (extent, strides in texels, vec; the origins are the caller's).  `at`
// names the frame, `names` its three pitches in the errors.  A tightly packed surface is checked as rows of pitch = width: the
// sized launch addresses it that way.  *packed_span: only that check failed -- the caller refuses unless the call is uniform.
int composite_frame_pitches(meao_ctx *ctx, const std::string &at, const char *const names[3], const meao_target_extent &e, int32_t color_format,
                            bool has_gbuffer0, CompositeSizedFrame *out, std::string *packed_span)
{
    const uint64_t elem[3] = {ao_elem(ctx->cfg), color_elem(color_format), 4};
    const uint64_t pitch[3] = {e.ao_pitch, e.color_pitch, has_gbuffer0 ? e.gbuffer0_pitch : 0};
    int32_t rows[3] = {e.width, e.width, e.width};
    for (int k = 0; k < (has_gbuffer0 ? 3 : 2); ++k) {
        if (pitch[k] != 0) {
            const int rc = pitch_texels_of(ctx, e.width, e.height, pitch[k], elem[k], (at + names[k]).c_str(), &rows[k]);
            if (rc != MEAO_OK) return rc;
        } else if (static_cast<uint64_t>(e.width) * e.height * elem[k] > 0xffffffffull && packed_span->empty()) {
            *packed_span = at + names[k] + ": a frame spans more than 2^32 - 1 bytes (tightly packed frames of a sized launch are rows like any other)";
        }
    }
    out->w = e.width; out->h = e.height;
    out->ao_stride = static_cast<uint32_t>(rows[0]); out->color_stride = static_cast<uint32_t>(rows[1]); out->gbuffer0_stride = static_cast<uint32_t>(rows[2]);
    // this frame's own form: colour base and rows whole 16-byte accesses, AO base and rows whole lanes of AO texels
    const uint32_t lane = color_lane_texels(color_format);
    out->vec = aligned_to(out->color, 16) && static_cast<uint64_t>(rows[1]) * elem[1] % 16 == 0 &&
               reinterpret_cast<uintptr_t>(out->ao) % (lane * elem[0]) == 0 && static_cast<uint32_t>(rows[0]) % lane == 0;
    return MEAO_OK;
}

// A uniform call's targets as meao_composite_batch takes them: extents[0]'s pitches for every frame
CompositeTargets uniform_targets(const CompositeTargets &t)
{
    CompositeTargets same = t;
    same.extents = nullptr;
    same.ao_pitch = t.extents[0].ao_pitch; same.color_pitch = t.extents[0].color_pitch; same.gbuffer0_pitch = t.extents[0].gbuffer0_pitch;
    return same;
}

// The checks of meao_composite_batch_extents under the name `fn` (t.extents set; t's three pitches are not read).  Touches
// nothing.  On success either *uniform -- every extent is the context's size and all frames share their strides: the call is
// meao_composite_batch with *pitch -- or entries[0 .. n) are the frames of the sized launch.
int composite_batch_extents_validate(meao_ctx *ctx, const char *fn, const CompositeTargets &t, CompositeSizedFrame *entries, bool *uniform,
                                     CompositePitches *pitch)
{
    if (!ctx || !t.ao || !t.color || !t.extents) return MEAO_ERR_INVALID_ARGUMENT;
    const std::string name(fn);
    if (t.n < 1 || t.n > ctx->cfg.max_batch) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, name + ": n must be 1..max_batch");
    if (t.mode < MEAO_COMPOSITE_MULTIPLY || t.mode > MEAO_COMPOSITE_DEBUG) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, name + ": unknown mode");
    if (t.mode == MEAO_COMPOSITE_AMBIENT_ONLY && !t.gbuffer0)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, name + ": gbuffer0_rgba8: AMBIENT_ONLY needs the GBuffer0 targets");
    for (int f = 0; f < t.n; ++f)
        if (!t.ao[f] || !t.color[f] || (t.mode == MEAO_COMPOSITE_AMBIENT_ONLY && !t.gbuffer0[f]))
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT,
                        name + ": frame " + std::to_string(f) + ": " + (!t.ao[f] ? "ao" : !t.color[f] ? "color" : "gbuffer0_rgba8") + ": null frame pointer");
    if (color_elem(t.color_format) == 0) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, name + ": color_format: not a meao_color_format");
    static const char *const in_extent[3] = {".ao_pitch", ".color_pitch", ".gbuffer0_pitch"};
    std::string packed_span;
    *uniform = true;
    for (int f = 0; f < t.n; ++f) {
        const meao_target_extent &e = t.extents[f];
        const std::string idx = "[" + std::to_string(f) + "]", at = name + ": extents" + idx;
        if (!size_valid(e.width, e.height)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, at + ".width/height out of range [1, 32768]");
        entries[f] = CompositeSizedFrame{};
        entries[f].ao = t.ao[f]; entries[f].color = t.color[f]; entries[f].gbuffer0 = t.gbuffer0 ? t.gbuffer0[f] : nullptr;
        // (the shaded call's colour and GBuffer0 pitches are arguments of their own: color_pitch[f], gbuffer0_pitch[f])
        const std::string color_name = name + ": color_pitch" + idx, g_name = name + ": gbuffer0_pitch" + idx;
        int rc;
        if (t.from_arrays) {
            const std::string ao_name = at + ".ao_pitch";
            const char *const names[3] = {ao_name.c_str(), color_name.c_str(), g_name.c_str()};
            rc = composite_frame_pitches(ctx, std::string(), names, e, t.color_format, t.gbuffer0 != nullptr, &entries[f], &packed_span);
        } else {
            rc = composite_frame_pitches(ctx, at, in_extent, e, t.color_format, t.gbuffer0 != nullptr, &entries[f], &packed_span);
        }
        if (rc != MEAO_OK) return rc;
        const CompositeSizedFrame &s = entries[f], &s0 = entries[0];
        *uniform = *uniform && e.width == ctx->cfg.width && e.height == ctx->cfg.height && s.ao_stride == s0.ao_stride &&
                   s.color_stride == s0.color_stride && (!t.gbuffer0 || s.gbuffer0_stride == s0.gbuffer0_stride);
    }
    if (*uniform) return composite_batch_validate(ctx, fn, uniform_targets(t), pitch);      // by its own rules: a packed frame there is not rows
    if (!packed_span.empty()) return fail(ctx, MEAO_ERR_UNSUPPORTED, packed_span);
    return MEAO_OK;
}

// The sized batched composite: the validated frames entries[0 .. n) in ONE composite_kernel launch on `stream`, through a slot
// of the context's sized table ring (the lease, arm and copy-then-launch discipline of composite_batch_launch).
int composite_batch_extents_launch(meao_ctx *ctx, const CompositeTargets &t, const CompositeSizedFrame *entries, hipStream_t stream)
{
    TableRing<CompositeSizedFrame, 8>::Lease lease;
    const int rc = ctx->comp_sized_ring.acquire(ctx, stream, &lease);
    if (rc != MEAO_OK) return rc;
    CompositeSizedFrame *stage = lease.host();
    for (int f = 0; f < t.n; ++f) stage[f] = entries[f];
    const int blocks = composite_sized_plan(stage, t.n, t.color_format);     // each frame's lanes per row; the largest frame's workgroups
    CompositeArgs ca{};
    ca.mode = t.mode;
    ca.color_format = t.color_format;
    ca.sized = lease.device();
    lease.arm();       // the slot is handed back guarded whatever happens from here: the copy may be in flight
    hipError_t e = hipMemcpyAsync(lease.device(), stage, sizeof(CompositeSizedFrame) * t.n, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = launch_composite_sized(ca, ctx->cfg.ao_format, stream, t.n, blocks);
    if (e != hipSuccess) return fail_hip(ctx, e, "composite_batch_extents_launch");
    return MEAO_OK;
}

}  // namespace

int meao::flush_pending_composite(meao_ctx *ctx, hipStream_t stream)
{
    CompositeBatchArgs &pc = ctx->pending_comp;
    const int frames = pc.frames;
    pc.frames = 0;
    for (int f = 0; f < frames; ++f) {
        CompositeArgs ca{};
        ca.ao = pc.ao[f]; ca.color = pc.color[f]; ca.gbuffer0 = pc.gbuffer0[f];
        ca.pixels = pc.pixels; ca.mode = pc.mode;
        ca.pitch = pc.pitch;       // the waiting batch remembers its pitches (meao_composite_enqueue_pitched)
        ca.color_format = ctx->pending_comp_format;     // ... and its colour format (meao_composite_enqueue_format)
        MEAO_HIP(ctx, launch_composite(ca, ctx->cfg.ao_format, stream));
    }
    return MEAO_OK;
}

int meao::composite_enqueue_internal(meao_ctx *ctx, const char *fn, const CompositeTargets &t, bool validate_only)
{
    CompositePitches pitch{};
    int rc = composite_enqueue_validate(ctx, fn, t, &pitch);
    if (rc != MEAO_OK || validate_only) return rc;     // a refused enqueue leaves a waiting batch waiting, untouched
    rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    if (ctx->pending_comp.frames > 0) {        // one batch can wait at a time: the older one runs now, in order
        rc = flush_pending_composite(ctx, ctx->pending_stream);
        if (rc != MEAO_OK) return rc;
    }
    ctx->pending_stream = ctx->last.stream;    // the stream of the execute that (by contract) produced ao[f]
    CompositeBatchArgs &pc = ctx->pending_comp;
    for (int f = 0; f < t.n; ++f) {
        pc.ao[f] = t.ao[f];
        pc.color[f] = t.color[f];
        pc.gbuffer0[f] = t.gbuffer0 ? t.gbuffer0[f] : nullptr;
        pitch.vec = pitch.vec && composite_vec_base(ctx, t.ao[f], t.color[f], t.color_format);      // one form for the batch
    }
    pc.pixels = static_cast<int64_t>(ctx->cfg.width) * ctx->cfg.height;
    pc.mode = t.mode;
    pc.frames = t.n;
    pc.pitch = pitch;
    ctx->pending_comp_format = t.color_format;
    return MEAO_OK;
}

int meao::execute_batch_shaded_internal(meao_ctx *ctx, const char *fn, const FrameSet &fs, const CompositeTargets &targets, meao_stream stream_,
                                        bool validate_only)
{
    if (!ctx || !fs.depth || !fs.out || !targets.color) return MEAO_ERR_INVALID_ARGUMENT;
    // both halves' checks before anything is enqueued: a refused call launches nothing
    int32_t depth_rows = 0, out_rows = 0;
    int rc = validate_execute_batch(ctx, fs, &depth_rows, &out_rows);
    if (rc != MEAO_OK) return fail(ctx, rc, std::string(fn) + ": " + ctx->err);      // the execute half's message, under this call's name
    CompositeTargets t = targets;      // the composite reads what the execute writes
    t.n = fs.n; t.ao = fs.out; t.ao_pitch = fs.out_pitch;
    CompositePitches pitch{};
    rc = composite_batch_validate(ctx, fn, t, &pitch);
    if (rc != MEAO_OK || validate_only) return rc;
    rc = execute_batch_internal(ctx, fs, stream_, false);
    if (rc != MEAO_OK) return rc;
    // behind the last AO kernel on the same stream (ctx->last.stream is the one the execute just ran on)
    return composite_batch_launch(ctx, t, pitch, ctx->last.stream);
}

int meao::execute_batch_extents_shaded_internal(meao_ctx *ctx, const char *fn, const FrameSet &fs, const CompositeTargets &targets, meao_stream stream_,
                                                bool validate_only)
{
    if (!ctx || !fs.depth || !fs.out || !fs.extents || !targets.color || !targets.extents) return MEAO_ERR_INVALID_ARGUMENT;
    // both halves' checks before anything is enqueued: a refused call launches nothing
    int32_t depth_rows[MEAO_MAX_BATCH], out_rows[MEAO_MAX_BATCH];
    bool uniform_execute = false;
    int rc = validate_execute_batch_extents(ctx, fs, depth_rows, out_rows, &uniform_execute);
    if (rc != MEAO_OK) return fail(ctx, rc, std::string(fn) + ": " + ctx->err);      // the execute half's message, under this call's name
    CompositeTargets t = targets;      // the composite reads what the execute writes
    t.n = fs.n; t.ao = fs.out;
    CompositeSizedFrame entries[MEAO_MAX_BATCH];
    CompositePitches pitch{};
    bool uniform = false;              // each half classifies itself
    rc = composite_batch_extents_validate(ctx, fn, t, entries, &uniform, &pitch);
    if (rc != MEAO_OK || validate_only) return rc;
    rc = execute_batch_internal(ctx, fs, stream_, false);
    if (rc != MEAO_OK) return rc;
    // behind the last AO kernel on the same stream (ctx->last.stream is the one the execute just ran on)
    if (uniform) return composite_batch_launch(ctx, uniform_targets(t), pitch, ctx->last.stream);
    return composite_batch_extents_launch(ctx, t, entries, ctx->last.stream);
}

// ------------------------------------------------------------------------------------------
extern "C" {

int32_t meao_composite(meao_ctx *ctx, int32_t mode, const void *ao, void *color_rgba16f, void *gbuffer0_rgba8,
                       int32_t loc, meao_stream stream_)
{
    return composite_single(ctx, "meao_composite", mode, ao, 0, color_rgba16f, MEAO_COLOR_RGBA16F, 0, gbuffer0_rgba8, 0, loc, stream_);
}

int32_t meao_composite_pitched(meao_ctx *ctx, int32_t mode, const void *ao, uint64_t ao_pitch, void *color_rgba16f, uint64_t color_pitch,
                               void *gbuffer0_rgba8, uint64_t gbuffer0_pitch, int32_t loc, meao_stream stream_)
{
    return composite_single(ctx, "meao_composite_pitched", mode, ao, ao_pitch, color_rgba16f, MEAO_COLOR_RGBA16F, color_pitch, gbuffer0_rgba8,
                            gbuffer0_pitch, loc, stream_);
}

int32_t meao_composite_format(meao_ctx *ctx, int32_t mode, const void *ao, uint64_t ao_pitch, void *color, int32_t color_format,
                              uint64_t color_pitch, void *gbuffer0_rgba8, uint64_t gbuffer0_pitch, int32_t loc, meao_stream stream_)
{
    return composite_single(ctx, "meao_composite_format", mode, ao, ao_pitch, color, color_format, color_pitch, gbuffer0_rgba8, gbuffer0_pitch,
                            loc, stream_);
}

int32_t meao_composite_enqueue(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, void *const *color_rgba16f,
                               void *const *gbuffer0_rgba8)
{
    return composite_enqueue_internal(ctx, "meao_composite_enqueue", CompositeTargets{mode, n, ao, 0, color_rgba16f, MEAO_COLOR_RGBA16F, 0, gbuffer0_rgba8, 0},
                                      false);
}

int32_t meao_composite_enqueue_pitched(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                       void *const *color_rgba16f, uint64_t color_pitch, void *const *gbuffer0_rgba8,
                                       uint64_t gbuffer0_pitch)
{
    return composite_enqueue_internal(ctx, "meao_composite_enqueue_pitched",
                                      CompositeTargets{mode, n, ao, ao_pitch, color_rgba16f, MEAO_COLOR_RGBA16F, color_pitch, gbuffer0_rgba8, gbuffer0_pitch},
                                      false);
}

int32_t meao_composite_enqueue_format(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch, void *const *color,
                                      int32_t color_format, uint64_t color_pitch, void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch)
{
    return composite_enqueue_internal(ctx, "meao_composite_enqueue_format",
                                      CompositeTargets{mode, n, ao, ao_pitch, color, color_format, color_pitch, gbuffer0_rgba8, gbuffer0_pitch}, false);
}

int32_t meao_composite_pending(const meao_ctx *ctx, int32_t *out_frames)
{
    if (!ctx || !out_frames) return MEAO_ERR_INVALID_ARGUMENT;
    *out_frames = ctx->pending_comp.frames;
    return MEAO_OK;
}

int32_t meao_composite_flush(meao_ctx *ctx, meao_stream stream_)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    if (ctx->pending_comp.frames == 0) return MEAO_OK;
    return flush_pending_composite(ctx, stream_ ? static_cast<hipStream_t>(stream_) : ctx->pending_stream);
}

int32_t meao_composite_batch(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch, void *const *color,
                             int32_t color_format, uint64_t color_pitch, void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch,
                             meao_stream stream_)
{
    const CompositeTargets t{mode, n, ao, ao_pitch, color, color_format, color_pitch, gbuffer0_rgba8, gbuffer0_pitch};
    CompositePitches pitch{};
    int rc = composite_batch_validate(ctx, "meao_composite_batch", t, &pitch);
    if (rc != MEAO_OK) return rc;
    rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    return composite_batch_launch(ctx, t, pitch, stream_ ? static_cast<hipStream_t>(stream_) : ctx->own_stream);
}

int32_t meao_execute_batch_shaded(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch, void *const *ao_out,
                                  uint64_t ao_pitch, const meao_params *params, int32_t mode, void *const *color, int32_t color_format,
                                  uint64_t color_pitch, void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch, meao_stream stream_)
{
    return execute_batch_shaded_internal(ctx, "meao_execute_batch_shaded",
                                         FrameSet{n, depth, depth_pitch, MEAO_MEM_DEVICE, ao_out, ao_pitch, MEAO_MEM_DEVICE, params},
                                         CompositeTargets{mode, n, nullptr, 0, color, color_format, color_pitch, gbuffer0_rgba8, gbuffer0_pitch}, stream_, false);
}

int32_t meao_composite_batch_extents(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, void *const *color, int32_t color_format,
                                     void *const *gbuffer0_rgba8, const meao_target_extent *extents, meao_stream stream_)
{
    static const char fn[] = "meao_composite_batch_extents";
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    if (!ao || !color || !extents) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": ao, color or extents is null");
    CompositeTargets t{mode, n, ao, 0, color, color_format, 0, gbuffer0_rgba8, 0};
    t.extents = extents;
    CompositeSizedFrame entries[MEAO_MAX_BATCH];
    CompositePitches pitch{};
    bool uniform = false;
    int rc = composite_batch_extents_validate(ctx, fn, t, entries, &uniform, &pitch);
    if (rc != MEAO_OK) return rc;
    rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    hipStream_t stream = stream_ ? static_cast<hipStream_t>(stream_) : ctx->own_stream;
    if (uniform) return composite_batch_launch(ctx, uniform_targets(t), pitch, stream);
    return composite_batch_extents_launch(ctx, t, entries, stream);
}

int32_t meao_execute_batch_extents_shaded(meao_ctx *ctx, int32_t n, const void *const *depth, void *const *ao_out, const meao_extent *extents,
                                          const meao_params *params, int32_t mode, void *const *color, int32_t color_format,
                                          const uint64_t *color_pitch, void *const *gbuffer0_rgba8, const uint64_t *gbuffer0_pitch, meao_stream stream_)
{
    static const char fn[] = "meao_execute_batch_extents_shaded";
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    if (!depth || !ao_out || !extents || !color)
        return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, std::string(fn) + ": depth, ao_out, extents or color is null");
    FrameSet fs{n, depth, 0, MEAO_MEM_DEVICE, ao_out, 0, MEAO_MEM_DEVICE, params};
    fs.extents = extents;
    meao_target_extent target[MEAO_MAX_BATCH];      // (an n out of range is refused before any entry is read)
    for (int32_t f = 0; f < n && f < MEAO_MAX_BATCH; ++f) target[f] = target_extent_of(extents[f], color_pitch, gbuffer0_pitch, f);
    CompositeTargets t{mode, n, nullptr, 0, color, color_format, 0, gbuffer0_rgba8, 0};
    t.extents = target; t.from_arrays = true;
    return execute_batch_extents_shaded_internal(ctx, fn, fs, t, stream_, false);
}

}  // extern "C"
