// meao_api.cpp -- the C ABI of libmeao_hip.so (include/meao.h): context lifecycle, parameters, queries, profiling and tracing.
// The calls that launch the pipeline live in meao_execute.cpp, the composites in meao_composite.cpp, the intermediates in
// meao_debug.cpp.  No CPU fallback exists anywhere in this library: without a gfx950 device meao_create fails with
// MEAO_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "meao_ctx.hpp"

using namespace meao;

namespace {

thread_local std::string g_last_error;   // for failures that have no context (meao_create)

bool config_valid(const meao_config &c, std::string *why)
{
    if (!size_valid(c.width, c.height)) { *why = "width/height out of range [1, 32768]"; return false; }
    if (c.num_levels < 1 || c.num_levels > 4) { *why = "num_levels must be 1..4"; return false; }
    if (c.ao_format != MEAO_AO_R8 && c.ao_format != MEAO_AO_F16) { *why = "unknown ao_format"; return false; }
    if (c.f16_rounding != MEAO_F16_RTZ_CLAMP && c.f16_rounding != MEAO_F16_RTNE) { *why = "unknown f16_rounding"; return false; }
    if (c.max_batch < 1 || c.max_batch > MEAO_MAX_BATCH) { *why = "max_batch must be 1..MEAO_MAX_BATCH"; return false; }
    if (c.depth_format < MEAO_DEPTH_F32 || c.depth_format > MEAO_DEPTH_LINEAR_F16) { *why = "unknown depth_format"; return false; }
    if (c.hq_levels < 0 || c.hq_levels > c.num_levels) { *why = "hq_levels must be 0..num_levels"; return false; }
    if (c.sample_set != MEAO_SAMPLES_CHECKER && c.sample_set != MEAO_SAMPLES_EXHAUSTIVE) { *why = "unknown sample_set"; return false; }
    if (c.pipelined != 0 && c.pipelined != 1) { *why = "pipelined must be 0 or 1"; return false; }
    return true;
}

SlotLayout layout_slot(const Plan &p, const meao_config &cfg, bool two_ds_sets)
{
    SlotLayout l;
    uint64_t off = 0;
    auto take = [&](uint64_t bytes) { const uint64_t o = off; off = align_up(off + bytes); return o; };
    auto px = [&](int k) { return static_cast<uint64_t>(p.mip[k].w) * p.mip[k].h; };
    for (int k = 1; k <= 4; ++k) l.off_ds_low[k - 1] = take(px(k) * 4);
    l.ds_set_bytes = off;
    if (two_ds_sets) off = 2 * off;          // second set: same layout, ds_set_bytes further
    for (int k = 1; k <= 4; ++k) l.off_occ[k - 1] = take(px(k) * ao_elem(cfg));
    for (int k = 1; k <= 3; ++k) l.off_comb[k - 1] = take(px(k) * ao_elem(cfg));
    for (int k = 1; k <= 4; ++k) l.off_hq[k - 1] = level_has_hq(cfg.num_levels, cfg.hq_levels, k) ? take(px(k) * ao_elem(cfg)) : 0;
    l.slot_bytes = off;
    return l;
}

void replan(meao_ctx *ctx)
{
    build_plan(ctx->cfg.width, ctx->cfg.height, ctx->cfg.num_levels, ctx->cfg.sample_set, ctx->prm, &ctx->plan);
    ctx->exact_rcp_div = exact_rcp_div_applicable(ctx->cfg, ctx->plan) ? 1 : 0;
}

void update_plan(meao_ctx *ctx)
{
    ctx->prefetch.withdraw(true);   // a prefetched downsample was computed with the old Z-buffer parameters
    replan(ctx);
}

// The reserved geometry, planned for layout_slot (only the level dimensions of the plan are read there).
SlotLayout layout_for(const meao_config &cfg, bool two_ds_sets, int32_t w, int32_t h)
{
    Plan plan{};
    for (int k = 0; k < kNumMips; ++k) plan.mip[k] = level_dims(w, h, k);
    return layout_slot(plan, cfg, two_ds_sets);
}

void release_buffers(meao_ctx *ctx)
{
    if (ctx->arena) (void)hipFree(ctx->arena);
    ctx->arena = nullptr;
    for (DeviceBuffer *b : {&ctx->stage_depth, &ctx->stage_out, &ctx->stage_view, &ctx->atlas_scratch, &ctx->pack_scratch}) b->release();
    ctx->last.frames = 0;
}

}  // namespace

int meao::fail(meao_ctx *ctx, int status, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    g_last_error = msg;
    return status;
}

int meao::fail_hip(meao_ctx *ctx, hipError_t e, const char *what)
{
    (void)hipGetLastError();
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), static_cast<int>(e));
    return fail(ctx, e == hipErrorOutOfMemory ? MEAO_ERR_OUT_OF_MEMORY : MEAO_ERR_HIP, buf);
}

void meao::note_sync(meao_ctx *ctx)
{
    if (ctx) ++ctx->sync_calls;
}

bool meao::size_valid(int32_t width, int32_t height) { return width >= 1 && height >= 1 && width <= 32768 && height <= 32768; }

int meao::use_device(meao_ctx *ctx)
{
    MEAO_HIP(ctx, hipSetDevice(ctx->cfg.device));
    return MEAO_OK;
}

// Divides on the path: 1/LoResDB, 1/centre depth, {9,3,1,3}/(|dHi-dLo| + tol), (HiAO*sum)/total.
// The exact v_rcp_f32 sequences need their operands inside verified ranges.  The DATA side of that
// (every linear depth in [2^-24, 2^20] or the sky value, finite, not NaN) is checked on the device: per frame
// by the downsample pass for the texels the levels are made of (nice_denominator; hostile frames take the IEEE
// bodies), per lane by the full-resolution upsample for the texels it linearizes itself.  The
// PARAMETER side is checked here: weights are <= 9/tol, total and sum are >= noise strength.
bool meao::exact_rcp_div_applicable(const meao_config &c, const Plan &plan)
{
    if (c.f16_rounding != MEAO_F16_RTZ_CLAMP) return false;               // RTNE stores inf for sky
    for (int k = 0; k < 4; ++k) {
        const meao_upsample_constants &u = plan.upsample[k];
        if (!(u.upsample_tolerance >= 0x1p-44f && u.upsample_tolerance <= 0x1p20f)) return false;  // weights <= 9 * 2^44
        if (!(u.noise_filter_strength >= 0x1p-30f && u.noise_filter_strength <= 0x1p50f)) return false;
    }
    return true;
}

// The new geometry is planned on the side and its arena allocated BEFORE anything of the context changes: on failure the
// context is untouched -- geometry, buffers and a ready prefetch all stay as they were.
int meao::reallocate(meao_ctx *ctx, const meao_config &cfg, bool two_ds_sets, int32_t cap_w, int32_t cap_h)
{
    const SlotLayout lay = layout_for(cfg, two_ds_sets, cap_w > 0 ? cap_w : cfg.width, cap_h > 0 ? cap_h : cfg.height);
    char *fresh = nullptr;
    hipError_t e;
    ++ctx->arena_allocs;
#if MEAO_TESTING
    if (ctx->debug_fail_allocs > 0) {      // fault injection: exists only in the `testhooks` variant library (-DMEAO_TESTING=1)
        --ctx->debug_fail_allocs;
        e = hipErrorOutOfMemory;
    } else
#endif
    {
        e = hipMalloc(reinterpret_cast<void **>(&fresh), lay.slot_bytes * cfg.max_batch);
    }
    if (e != hipSuccess) return fail_hip(ctx, e, "hipMalloc (intermediates)");
    ctx->cfg = cfg;
    ctx->two_ds_sets = two_ds_sets;
    ctx->cap_w = cap_w; ctx->cap_h = cap_h;
    update_plan(ctx);           // drops a ready prefetch: it refers to the old arena
    ctx->lay = lay;
    release_buffers(ctx);
    ctx->arena = fresh;
    return MEAO_OK;
}

void meao::Profiler::fold()
{
    for (int r = 0; r < ring_fill; ++r) {
        for (int k = 0; k < kProfSlots; ++k) {
            if (!(ran_mask[r] >> k & 1u)) continue;
            hipEvent_t a = events[(r * kProfSlots + k) * 2], b = events[(r * kProfSlots + k) * 2 + 1];
            note_sync(owner);
            (void)hipEventSynchronize(b);
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, a, b) != hipSuccess) continue;
            pass_ms_sum[k] += ms;
            ++pass_samples[k];
        }
        ++executes_profiled;
    }
    ring_fill = 0;
}

// ------------------------------------------------------------------------------------------
extern "C" {

int32_t meao_abi_version(void) { return MEAO_ABI_VERSION; }

const char *meao_status_string(int32_t status)
{
    switch (status) {
    case MEAO_OK: return "ok";
    case MEAO_ERR_INVALID_ARGUMENT: return "invalid argument";
    case MEAO_ERR_HIP: return "HIP runtime error";
    case MEAO_ERR_OUT_OF_MEMORY: return "out of memory";
    case MEAO_ERR_UNSUPPORTED: return "unsupported";
    case MEAO_ERR_NO_DEVICE: return "no gfx950 device (there is no CPU fallback)";
    case MEAO_ERR_BUFFER_TOO_SMALL: return "destination buffer too small";
    default: return "unknown status";
    }
}

void meao_default_config(meao_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = sizeof *cfg;
    cfg->device = 0;
    cfg->width = 1920;
    cfg->height = 1080;
    cfg->num_levels = 4;
    cfg->ao_format = MEAO_AO_R8;
    cfg->f16_rounding = MEAO_F16_RTZ_CLAMP;
    cfg->max_batch = 1;
    cfg->depth_format = MEAO_DEPTH_F32;
    cfg->pipelined = 0;
}

void meao_default_params(meao_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->noise_filter_tolerance = 0.0f;   // AO.cs:20
    p->blur_tolerance = -4.6f;          // AO.cs:28
    p->upsample_tolerance = -12.0f;     // AO.cs:36
    p->thickness_modifier = 1.0f;       // AO.cs:44
    p->intensity = 1.0f;                // AO.cs:52
    p->near_clip = 0.3f;                // Unity camera defaults
    p->far_clip = 1000.0f;
    p->proj00 = 0.9742786f;             // fovY 60 deg at 16:9
    p->reversed_z = 1;
}

int32_t meao_level_dims(int32_t width, int32_t height, int32_t level, int32_t *out_w, int32_t *out_h)
{
    if (width < 1 || height < 1 || level < 0 || level >= kNumMips || !out_w || !out_h)
        return MEAO_ERR_INVALID_ARGUMENT;
    const Dims d = level_dims(width, height, level);
    *out_w = d.w;
    *out_h = d.h;
    return MEAO_OK;
}

int32_t meao_zbuffer_params(const meao_params *p, float out[4])
{
    if (!p || !out || !params_valid(*p)) return MEAO_ERR_INVALID_ARGUMENT;
    zbuffer_params(*p, out);
    return MEAO_OK;
}

int32_t meao_render_constants_for(int32_t width, int32_t height, const meao_params *p, int32_t level,
                                  meao_render_constants *out)
{
    if (width < 1 || height < 1 || !p || !out || level < 1 || level > 4 || !params_valid(*p))
        return MEAO_ERR_INVALID_ARGUMENT;
    render_constants(width, height, *p, level, true, MEAO_SAMPLES_CHECKER, out);
    return MEAO_OK;
}

int32_t meao_render_constants_variant(int32_t width, int32_t height, const meao_params *p, int32_t level,
                                      int32_t source_tiled, int32_t sample_set, meao_render_constants *out)
{
    if (width < 1 || height < 1 || !p || !out || level < 1 || level > 4 || !params_valid(*p))
        return MEAO_ERR_INVALID_ARGUMENT;
    if (sample_set != MEAO_SAMPLES_CHECKER && sample_set != MEAO_SAMPLES_EXHAUSTIVE) return MEAO_ERR_INVALID_ARGUMENT;
    render_constants(width, height, *p, level, source_tiled != 0, sample_set, out);
    return MEAO_OK;
}

int32_t meao_upsample_constants_for(int32_t width, int32_t height, const meao_params *p, int32_t low_level,
                                    meao_upsample_constants *out)
{
    if (width < 1 || height < 1 || !p || !out || low_level < 1 || low_level > 4 || !params_valid(*p))
        return MEAO_ERR_INVALID_ARGUMENT;
    upsample_constants(width, height, *p, low_level, out);
    return MEAO_OK;
}

int32_t meao_describe_buffer(const meao_config *cfg, int32_t debug_id, meao_desc *out)
{
    std::string why;
    if (!cfg || !out || !config_valid(*cfg, &why)) return MEAO_ERR_INVALID_ARGUMENT;
    return describe_buffer(cfg->width, cfg->height, cfg->ao_format, debug_id, out) ? MEAO_OK
                                                                                   : MEAO_ERR_INVALID_ARGUMENT;
}

int32_t meao_algorithmic_bytes(const meao_config *cfg, uint64_t bytes[MEAO_NUM_PASSES])
{
    std::string why;
    if (!cfg || !bytes || !config_valid(*cfg, &why)) return MEAO_ERR_INVALID_ARGUMENT;
    algorithmic_bytes(cfg->width, cfg->height, cfg->num_levels, cfg->hq_levels, cfg->ao_format, cfg->depth_format, bytes);
    return MEAO_OK;
}

int32_t meao_create(const meao_config *cfg, meao_ctx **out_ctx)
{
    if (out_ctx) *out_ctx = nullptr;
    if (!cfg || !out_ctx) return fail(nullptr, MEAO_ERR_INVALID_ARGUMENT, "meao_create: null argument");
    if (cfg->struct_size != sizeof(meao_config))
        return fail(nullptr, MEAO_ERR_INVALID_ARGUMENT, "meao_create: struct_size mismatch (ABI)");
    std::string why;
    if (!config_valid(*cfg, &why)) return fail(nullptr, MEAO_ERR_INVALID_ARGUMENT, "meao_create: " + why);

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, MEAO_ERR_NO_DEVICE, "meao_create: no HIP device visible (no CPU fallback exists)");
    }
    if (cfg->device < 0 || cfg->device >= count)
        return fail(nullptr, MEAO_ERR_INVALID_ARGUMENT, "meao_create: device ordinal out of range");
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, cfg->device)) != hipSuccess) return fail_hip(nullptr, e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, MEAO_ERR_NO_DEVICE,
                    std::string("meao_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

    meao_ctx *ctx = new (std::nothrow) meao_ctx();
    if (!ctx) return fail(nullptr, MEAO_ERR_OUT_OF_MEMORY, "meao_create: host allocation failed");
    ctx->cfg = *cfg;
    ctx->profiler.owner = ctx;
    meao_default_params(&ctx->prm);
    int rc = use_device(ctx);
    if (rc == MEAO_OK) {
        e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
        if (e != hipSuccess) rc = fail_hip(ctx, e, "hipStreamCreateWithFlags");
    }
    if (rc == MEAO_OK) {
        // hostile-depth flags: 2 downsample sets x MEAO_MAX_BATCH frames, zero = never hostile (generations start at 1)
        const size_t bytes = 2 * MEAO_MAX_BATCH * sizeof(uint32_t);
        e = hipMalloc(reinterpret_cast<void **>(&ctx->hostile), bytes);
        if (e == hipSuccess) e = hipMemset(ctx->hostile, 0, bytes);
        if (e != hipSuccess) rc = fail_hip(ctx, e, "hipMalloc (hostile flags)");
    }
    if (rc == MEAO_OK) {
        // per-frame constants (meao_execute_batch_params): the plans and the ring of FrameArgs tables
        ctx->frame_plan.resize(MEAO_MAX_BATCH);
        ctx->prefetch.next.plan.resize(MEAO_MAX_BATCH);
        if ((e = ctx->frame_ring.create(cfg->max_batch)) != hipSuccess) rc = fail_hip(ctx, e, "per-frame constant tables");
    }
    // the batched composite's frame tables (meao_composite_batch): the same kind of ring
    if (rc == MEAO_OK && (e = ctx->comp_ring.create(cfg->max_batch)) != hipSuccess) rc = fail_hip(ctx, e, "batched composite tables");
    if (rc == MEAO_OK && (e = ctx->comp_sized_ring.create(cfg->max_batch)) != hipSuccess) rc = fail_hip(ctx, e, "sized composite tables");
    // cfg.pipelined: the second downsample set exists from the start, so meao_prefetch_batch never re-allocates
    if (rc == MEAO_OK) rc = reallocate(ctx, *cfg, cfg->pipelined != 0, 0, 0);
    if (rc != MEAO_OK) {
        g_last_error = ctx->err;
        meao_destroy(ctx);
        return rc;
    }
    ctx->last.stream = ctx->own_stream;
    *out_ctx = ctx;
    return MEAO_OK;
}

int32_t meao_destroy(meao_ctx *ctx)
{
    if (!ctx) return MEAO_OK;
    int prev_device = -1;
    (void)hipGetDevice(&prev_device);
    (void)hipSetDevice(ctx->cfg.device);
    // A composite batch still waiting is DISCARDED (meao.h): its targets are caller memory whose lifetime has
    // typically ended by now (free the frames, then destroy); hosts that want it call meao_composite_flush first.
    ctx->pending_comp.frames = 0;
    note_sync(ctx);
    (void)hipDeviceSynchronize();
    release_buffers(ctx);
    if (ctx->counter) (void)hipFree(ctx->counter);
    if (ctx->hostile) (void)hipFree(ctx->hostile);
    ctx->frame_ring.destroy();
    ctx->comp_ring.destroy();
    ctx->comp_sized_ring.destroy();
    if (ctx->tracer.lib) (void)dlclose(ctx->tracer.lib);
    for (hipEvent_t ev : ctx->profiler.events) (void)hipEventDestroy(ev);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
    return MEAO_OK;
}

int32_t meao_resize(meao_ctx *ctx, int32_t width, int32_t height)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    meao_config c = ctx->cfg;
    c.width = width;
    c.height = height;
    std::string why;
    if (!config_valid(c, &why)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_resize: " + why);
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    if (ctx->pending_comp.frames > 0) {        // sized for the old geometry: run it now, where its AO frames were produced
        rc = flush_pending_composite(ctx, ctx->pending_stream);
        if (rc != MEAO_OK) return rc;
    }
    if (ctx->within_reservation(width, height)) {
        // Nothing moves: every buffer of a slot stays at the offset the reserved geometry gives it, and the launch arguments of
        // the next call are built from the new plan.  No allocation, no synchronisation, no launch: the stream orders the next
        // call behind the last one, as it orders any two executes of this context (they share the intermediates).
        ctx->cfg = c;
        replan(ctx);
        ctx->prefetch.resized_to(width, height);
        ctx->last.frames = 0;                  // the debug buffers of the last call are gone, as in every resize
        return MEAO_OK;
    }
    note_sync(ctx);
    MEAO_HIP(ctx, hipDeviceSynchronize());
    // on failure (e.g. out of memory) the context keeps its previous size, buffers and reservation; a reservation grows to cover
    // the new size
    const bool reserved = ctx->cap_w > 0;
    return reallocate(ctx, c, ctx->two_ds_sets, reserved ? std::max(ctx->cap_w, width) : 0, reserved ? std::max(ctx->cap_h, height) : 0);
}

int32_t meao_reserve(meao_ctx *ctx, int32_t max_width, int32_t max_height)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    const bool drop = max_width == 0 && max_height == 0;
    if (!drop) {
        if (!size_valid(max_width, max_height)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_reserve: max_width/max_height out of range [1, 32768]");
        if (max_width < ctx->cfg.width || max_height < ctx->cfg.height)
            return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_reserve: max_width/max_height: the reservation must cover the current size");
    }
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    note_sync(ctx);
    MEAO_HIP(ctx, hipDeviceSynchronize());
    // (a waiting composite batch stays: its surfaces are the caller's, and the size does not change)
    return reallocate(ctx, ctx->cfg, ctx->two_ds_sets, drop ? 0 : max_width, drop ? 0 : max_height);
}

int32_t meao_get_capacity(const meao_ctx *ctx, int32_t *out_width, int32_t *out_height)
{
    if (!ctx || !out_width || !out_height) return MEAO_ERR_INVALID_ARGUMENT;
    *out_width = ctx->cap_w;
    *out_height = ctx->cap_h;
    return MEAO_OK;
}

int32_t meao_reserve_bytes(const meao_config *cfg, int32_t max_width, int32_t max_height, uint64_t *out_bytes)
{
    std::string why;
    if (!cfg || !out_bytes || !config_valid(*cfg, &why) || !size_valid(max_width, max_height)) return MEAO_ERR_INVALID_ARGUMENT;
    *out_bytes = layout_for(*cfg, cfg->pipelined != 0, max_width, max_height).slot_bytes * static_cast<uint64_t>(cfg->max_batch);
    return MEAO_OK;
}

int32_t meao_set_params(meao_ctx *ctx, const meao_params *p)
{
    if (!ctx || !p) return MEAO_ERR_INVALID_ARGUMENT;
    if (p->struct_size != sizeof(meao_params)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_set_params: struct_size mismatch (ABI)");
    if (!params_valid(*p)) return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_set_params: non-finite or degenerate parameter");
    ctx->prm = *p;
    update_plan(ctx);
    return MEAO_OK;
}

int32_t meao_get_params(const meao_ctx *ctx, meao_params *out)
{
    if (!ctx || !out) return MEAO_ERR_INVALID_ARGUMENT;
    *out = ctx->prm;
    return MEAO_OK;
}

int32_t meao_get_config(const meao_ctx *ctx, meao_config *out)
{
    if (!ctx || !out) return MEAO_ERR_INVALID_ARGUMENT;
    *out = ctx->cfg;
    return MEAO_OK;
}

const char *meao_last_error(const meao_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int32_t meao_synchronize(meao_ctx *ctx, meao_stream stream)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    note_sync(ctx);
    MEAO_HIP(ctx, hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : ctx->last.stream));
    return MEAO_OK;
}

int32_t meao_hostile_frames(meao_ctx *ctx, uint64_t *out_mask)
{
    if (!ctx || !out_mask) return MEAO_ERR_INVALID_ARGUMENT;
    *out_mask = 0;
    if (ctx->last.frames == 0) return MEAO_OK;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    uint32_t words[MEAO_MAX_BATCH];
    MEAO_HIP(ctx, hipMemcpyAsync(words, ctx->hostile_of(ctx->prefetch.ds_cur), sizeof(uint32_t) * ctx->last.frames, hipMemcpyDeviceToHost,
                                 ctx->last.stream));
    note_sync(ctx);
    MEAO_HIP(ctx, hipStreamSynchronize(ctx->last.stream));
    for (int f = 0; f < ctx->last.frames; ++f)
        if (words[f] == ctx->prefetch.generation()) *out_mask |= uint64_t(1) << f;
    return MEAO_OK;
}

int32_t meao_set_profiling(meao_ctx *ctx, int32_t enable)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    Profiler &pr = ctx->profiler;
    if (enable && pr.events.empty()) {
        const int count = kProfileRing * kProfSlots * 2;
        pr.events.reserve(count);
        for (int i = 0; i < count; ++i) {
            hipEvent_t ev;
            // timing only: no system-scope fence (cache write-back + invalidate) when a record completes -- nothing synchronizes
            // with these events but hipEventElapsedTime
            MEAO_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableSystemFence));
            pr.events.push_back(ev);
        }
    }
    if (enable) {   // (re)start a measurement window
        pr.fold();
        std::memset(pr.pass_ms_sum, 0, sizeof pr.pass_ms_sum);
        std::memset(pr.pass_samples, 0, sizeof pr.pass_samples);
        pr.executes_profiled = 0;
    }
    pr.on = enable != 0;
    pr.period = enable > 1 ? enable : 1;
    pr.phase = 0;
    return MEAO_OK;
}

int32_t meao_get_pass_times(meao_ctx *ctx, float ms[MEAO_NUM_PASSES], int32_t *out_samples)
{
    if (!ctx || !ms) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    // the documented contract: the call returns after the stream of the last execute has drained (executes that recorded no
    // events -- meao_set_profiling(N > 1), PROFILE_PASS_MASK -- included; the timing events themselves carry no fence)
    note_sync(ctx);
    MEAO_HIP(ctx, hipStreamSynchronize(ctx->last.stream));
    Profiler &pr = ctx->profiler;
    pr.fold();
    // mean over the executes that actually ran the pass (a prefetched downsample does not dilute it)
    for (int k = 0; k < MEAO_NUM_PASSES; ++k)
        ms[k] = pr.pass_samples[k] ? static_cast<float>(pr.pass_ms_sum[k] / pr.pass_samples[k]) : 0.0f;
    if (out_samples) *out_samples = pr.executes_profiled;
    return MEAO_OK;
}

int32_t meao_set_tracing(meao_ctx *ctx, int32_t enable)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    Tracer &t = ctx->tracer;
    if (enable && !t.lib) {
        // rocprofv3 (rocprofiler-sdk) intercepts the roctx API of its own library; libroctx64.so is the
        // older roctracer one (rocprof v1/v2) with the same entry points
        static const char *const kCandidates[] = {"librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so",
                                                  "libroctx64.so", "/opt/rocm/lib/libroctx64.so"};
        void *lib = nullptr;
        for (const char *name : kCandidates)
            if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
        if (!lib) return fail(ctx, MEAO_ERR_UNSUPPORTED, "meao_set_tracing: no roctx library found (librocprofiler-sdk-roctx.so / libroctx64.so)");
        t.push = reinterpret_cast<int (*)(const char *)>(dlsym(lib, "roctxRangePushA"));
        t.pop = reinterpret_cast<int (*)()>(dlsym(lib, "roctxRangePop"));
        if (!t.push || !t.pop) {
            (void)dlclose(lib);
            t.push = nullptr; t.pop = nullptr;
            return fail(ctx, MEAO_ERR_UNSUPPORTED, "meao_set_tracing: roctxRangePushA / roctxRangePop missing");
        }
        t.lib = lib;
    }
    t.on = enable != 0;
    return MEAO_OK;
}

int32_t meao_debug_set(meao_ctx *ctx, int32_t key, int32_t value)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    Tuning &t = ctx->tuning;
    switch (key) {
    case MEAO_DEBUG_FUSE_COARSE_BLEND: t.fuse_coarse_blend = value != 0; break;
    case MEAO_DEBUG_NESTED_MAX_TILES: t.nested_max_tiles = value; break;
    case MEAO_DEBUG_RENDER_SMALL_MAX_TILES: t.render_small_max_tiles = value; break;
    case MEAO_DEBUG_FINAL_SMALL_MAX_TILES: t.final_small_max_tiles = value; break;
    case MEAO_DEBUG_DS_SMALL_MAX_TILES: t.ds_small_max_tiles = value; break;
    case MEAO_DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: t.next_ds_own_launch = value != 0; break;
    case MEAO_DEBUG_PROFILE_PASS_MASK: ctx->profiler.mask = value == 0 ? ~0u : static_cast<uint32_t>(value); break;
    case MEAO_DEBUG_BLEND_TALL_MIN_TILES:
        t.blend_tall_min_tiles = value <= 0 ? 0x7fffffff : value;
        t.blend_tall_forced = true;
        break;
    default: return fail(ctx, MEAO_ERR_INVALID_ARGUMENT, "meao_debug_set: unknown key");
    }
    return MEAO_OK;
}

#if MEAO_TESTING
// Fault injection for the resize / first-announcement error paths (tests/test_gpu_more.py): the next n allocations of
// intermediates fail with MEAO_ERR_OUT_OF_MEMORY.  Not declared in include/meao.h and not compiled into libmeao_hip.so:
// only the `testhooks` variant library (miniengineao_amd/build.py VARIANTS, -DMEAO_TESTING=1) exports it.
__attribute__((visibility("default"))) int32_t meao_test_fail_next_allocs(meao_ctx *ctx, int32_t n)
{
    if (!ctx) return MEAO_ERR_INVALID_ARGUMENT;
    ctx->debug_fail_allocs = n < 0 ? 0 : n;
    return MEAO_OK;
}

// out[0]: arena allocations attempted since meao_create (an injected failure counts); out[1]: synchronising HIP calls the
// context has made since then (device, stream and event synchronise).  What proves that a meao_resize inside a reservation
// neither allocates nor waits (tests/dynamic_resolution_testhooks_check.py).
__attribute__((visibility("default"))) int32_t meao_test_counters(const meao_ctx *ctx, uint64_t out[2])
{
    if (!ctx || !out) return MEAO_ERR_INVALID_ARGUMENT;
    out[0] = ctx->arena_allocs;
    out[1] = ctx->sync_calls;
    return MEAO_OK;
}
#endif

int32_t meao_selftest(meao_ctx *ctx, int32_t which, uint64_t *out_mismatches)
{
    if (!ctx || !out_mismatches || which < 0 || which > 9) return MEAO_ERR_INVALID_ARGUMENT;
    int rc = use_device(ctx);
    if (rc != MEAO_OK) return rc;
    if (!ctx->counter) MEAO_HIP(ctx, hipMalloc(reinterpret_cast<void **>(&ctx->counter), sizeof(unsigned long long)));
    MEAO_HIP(ctx, hipMemsetAsync(ctx->counter, 0, sizeof(unsigned long long), ctx->own_stream));
    MEAO_HIP(ctx, launch_selftest(which, ctx->counter, ctx->own_stream));
    unsigned long long host = 0;
    MEAO_HIP(ctx, hipMemcpyAsync(&host, ctx->counter, sizeof host, hipMemcpyDeviceToHost, ctx->own_stream));
    note_sync(ctx);
    MEAO_HIP(ctx, hipStreamSynchronize(ctx->own_stream));
    *out_mismatches = host;
    return MEAO_OK;
}

}  // extern "C"
