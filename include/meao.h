/*
 * meao.h -- C ABI of libmeao_hip.so: the MI355X-native (gfx950 / CDNA4) multi-scale
 * SSAO hot path of keijiro/MiniEngineAO.   depth in  ->  ambient-occlusion texture out.
 *
 * What this boundary replaces.  The reference has no FFI: the path sits behind the Unity
 * component MiniEngineAO.AmbientOcclusion (Assets/MiniEngineAO/AmbientOcclusion.cs, "AO.cs"
 * below), which records ten compute dispatches into a CommandBuffer
 * (AO.cs:496-531 RebuildCommandBuffers).  Every entry point below names the reference
 * lines it stands in for; INTEGRATION.md shows the C# [DllImport] stub and the
 * AmbientOcclusion wrapper a maintainer would add on the reference side.
 *
 * Conventions: plain C, no C++ or torch types; every function returns a meao_status
 * (0 = ok, negative = error) unless stated; no exception crosses the boundary; a context
 * is not thread-safe, distinct contexts are independent (no global state -- the reference's
 * shared statics AO.cs:136-137,592-593 are per-context here); one context per device.
 * The caller owns the input depth and output AO memory; the context owns every
 * intermediate and never allocates inside meao_execute*.
 */
#ifndef MEAO_H
#define MEAO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MEAO_API __attribute__((visibility("default")))
#else
#define MEAO_API
#endif

#define MEAO_ABI_VERSION 7
#define MEAO_MAX_BATCH 64      /* frames per batched launch */
#define MEAO_NUM_PASSES 7      /* downsample, render, upsample x4, render_hq (see meao_pass) */

typedef struct meao_ctx meao_ctx;
typedef void *meao_stream;     /* hipStream_t; NULL = the context's own stream */

typedef enum meao_status {
    MEAO_OK = 0,
    MEAO_ERR_INVALID_ARGUMENT = -1,
    MEAO_ERR_HIP = -2,            /* HIP runtime error; text via meao_last_error */
    MEAO_ERR_OUT_OF_MEMORY = -3,
    MEAO_ERR_UNSUPPORTED = -4,
    MEAO_ERR_NO_DEVICE = -5,      /* no gfx950 device visible: there is no CPU fallback */
    MEAO_ERR_BUFFER_TOO_SMALL = -6
} meao_status;

/* Storage of the AO targets.  R8 = the reference's FixedUAV / RenderTextureFormat.R8
 * (AO.cs:262-273,466-475): AO is quantised to 8 bits between every pass.  F16 = fp16 AO
 * storage (BASELINE config 5). */
typedef enum meao_ao_format { MEAO_AO_R8 = 0, MEAO_AO_F16 = 1 } meao_ao_format;

/* f32 -> f16 store conversion of the HalfUAV targets (AO.cs:454).  RTZ_CLAMP (round toward
 * zero, finite overflow -> 65504) is canonical; RTNE (overflow -> inf) is the other common
 * hardware behaviour.  Only matters for sky texels (1e5) and the last mantissa bit. */
typedef enum meao_f16_rounding { MEAO_F16_RTZ_CLAMP = 0, MEAO_F16_RTNE = 1 } meao_f16_rounding;

/* Numerics (one mode, no switch): bit-exact against the CPU oracle -- correctly rounded '/', explicit mad fusion only
 * (DESIGN.md section 2).  (ABI <= 5 had a FAST mode with raw 1-ulp reciprocals; it was outside the parity bar and is gone.) */
typedef enum meao_mem { MEAO_MEM_HOST = 0, MEAO_MEM_DEVICE = 1 } meao_mem;

/* Storage of the input depth buffer.  The reference first blits _CameraDepthTexture -- whatever
 * its format -- into an RFloat copy (Blit.shader:48-64 pass 0, AO.cs:608-614) unless D3D's
 * resolved depth is available; here the downsample kernel decodes the format on load, so that
 * pass does not exist.  UNORM formats decode to v / (2^n - 1), correctly rounded (what
 * SAMPLE_DEPTH_TEXTURE returns): UNORM16 = D16, UNORM24 = the low 24 bits of a 32-bit word
 * (D24S8 / D24X8; the high byte is ignored).  F16 decodes exactly.
 *
 * LINEAR_F32 / LINEAR_F16: linear view-space depth instead of a hardware depth buffer.  A texel is z along the camera axis in
 * the units of near_clip / far_clip (Unity's LinearEyeDepth; with far_clip = 1 it is Linear01Depth); f16 texels widen to f32
 * exactly.  Linear01 depth is dist = z * s, one f32 multiply rounded to nearest even, with s the f32 nearest to 1 / far_clip
 * (per call, or per frame under meao_execute_batch_params): when far_clip is a power of two, dist == z / far_clip exactly.
 * dist >= 1 (the far plane and beyond, +inf included) becomes 1e5f, the value the hardware formats give their far-plane
 * texel; every other value passes through unchanged (NaN, negatives, +-0, denormals take the IEEE-division bodies, and
 * meao_hostile_frames reports a frame whose level texels hold a non-sky dist that is NaN or outside [2^-24, 2^20]).  The
 * texels are decoded with far_clip alone; near_clip and reversed_z set only the padding of the level 1-2 atlases, as for every
 * format (Linearize of an out-of-range load: near_clip / far_clip with conventional Z, 1e5 with reversed Z), so a host passes
 * its camera's real values.  A prefetched downsample pass is reused when each frame's s matches.  meao_params validation is
 * unchanged.  So a linear frame equal to the Linearize of a hardware frame gives the hardware frame's results bit for bit.  Every entry point accepts them; HOST frames and pitches
 * use their element size (4 / 2 bytes).  They arrived without an ABI version change: libraries built before them reject
 * depth_format 4 and 5 at meao_create with MEAO_ERR_INVALID_ARGUMENT, which is how a host probes for support. */
typedef enum meao_depth_format {
    MEAO_DEPTH_F32 = 0, MEAO_DEPTH_UNORM16 = 1, MEAO_DEPTH_UNORM24 = 2, MEAO_DEPTH_F16 = 3,
    MEAO_DEPTH_LINEAR_F32 = 4, MEAO_DEPTH_LINEAR_F16 = 5
} meao_depth_format;

typedef enum meao_format { MEAO_FMT_F32 = 0, MEAO_FMT_F16 = 1, MEAO_FMT_UNORM8 = 2 } meao_format;

/* Sample set of the AO render.  CHECKER = what the reference dispatches (36 samples,
 * Render.compute:160-169).  EXHAUSTIVE = the shader's SAMPLE_EXHAUSTIVELY branch (68 samples, all
 * 12 table slots, Render.compute:144-159), which the reference's host never enables (AO.cs:709
 * "FIXME: should we support SAMPLE_EXHAUSTIVELY mode?"): the weight table is then the un-zeroed
 * AO.cs:696-707 table, normalised the same way. */
typedef enum meao_sample_set { MEAO_SAMPLES_CHECKER = 0, MEAO_SAMPLES_EXHAUSTIVE = 1 } meao_sample_set;

/* Buffers beyond the reference's 17 debug ids: the Render.main (wide) targets of the hq_levels
 * variant, OcclusionHQ1..4 (AO format, dims of L1..L4). */
#define MEAO_DEBUG_OCCLUSION_HQ1 18
#define MEAO_NUM_BUFFERS 21

/* Kernel launches of one frame/batch, in stream order. */
typedef enum meao_pass {
    MEAO_PASS_DOWNSAMPLE = 0,  /* Downsample1.main + Downsample2.main fused  (AO.cs:627-657): the four point-sampled levels.
                                * LinearDepth (Downsample1.compute:46) is not written: its one reader, Upsample.main, evaluates
                                * Linearize from the raw depth frame itself */
    MEAO_PASS_RENDER = 1,      /* Render.main_interleaved, all levels, one grid (AO.cs:519-522) */
    MEAO_PASS_UPSAMPLE_3 = 2,  /* Upsample.main_blendout L4 -> L3             (AO.cs:528).  With 4 levels and
                                * hq_levels = 0 it is evaluated inside the L3 -> L2 launch (each tile computes the
                                * window of Combined3 it reads; Combined3 is still written): no launch of its
                                * own, meao_get_pass_times reports 0 here and the joint time under UPSAMPLE_2 */
    MEAO_PASS_UPSAMPLE_2 = 3,  /* Upsample.main_blendout L3 -> L2             (AO.cs:529).  Small calls (frames x
                                * 64x32 tiles of L1 <= 1024, e.g. one 4K frame or up to four 1080p frames) evaluate it and L4 -> L3 inside
                                * the L2 -> L1 launch: 0 here and under UPSAMPLE_3, the joint time under UPSAMPLE_1 */
    MEAO_PASS_UPSAMPLE_1 = 4,  /* Upsample.main_blendout L2 -> L1             (AO.cs:530) */
    MEAO_PASS_UPSAMPLE_0 = 5,  /* Upsample.main          L1 -> L0 result      (AO.cs:531) */
    MEAO_PASS_RENDER_HQ = 6    /* Render.main (wide) on LowDepth<k>, all hq levels, one grid; launched
                                * right after MEAO_PASS_RENDER (cfg.hq_levels > 0 only) */
} meao_pass;

/* What DoLazyInitialization + RTHandle sizing fix per instance (AO.cs:440-476,276-281). */
typedef struct meao_config {
    uint32_t struct_size;   /* sizeof(meao_config), for ABI evolution */
    int32_t device;         /* HIP device ordinal */
    int32_t width, height;  /* camera.pixelWidth / pixelHeight (AO.cs:339-340) */
    int32_t num_levels;     /* 1..4; the reference always runs 4 (AO.cs:519-531) */
    int32_t ao_format;      /* meao_ao_format */
    int32_t f16_rounding;   /* meao_f16_rounding */
    int32_t max_batch;      /* 1..MEAO_MAX_BATCH frames resident per launch */
    int32_t depth_format;   /* meao_depth_format of the depth pointers given to meao_execute* */
    /* Variants present in the reference's shaders but never dispatched by its host (0 = reference): */
    int32_t hq_levels;      /* 0..num_levels.  The coarsest hq_levels levels additionally run
                             * Render.main (WIDE_SAMPLING, non-interleaved; Render.compute:22,27-29,
                             * 46-50) on LowDepth<k>, and the upsample that consumes level k becomes
                             * Upsample.main_premin / main_premin_blendout (Upsample.compute:23,25,58-60):
                             * LoResAO1 = min(LoResAO1, that render).  Wiring as in the Microsoft
                             * MiniEngine original (its quality levels = hq_levels 0..4). */
    int32_t sample_set;     /* meao_sample_set */
    int32_t pipelined;      /* 1: allocate the second set of downsample buffers at meao_create, so that
                             * meao_prefetch_batch never allocates or synchronises (streams of frames);
                             * 0 (default): the first meao_prefetch_batch call does it, once */
} meao_config;

/* The component's serialized properties (AO.cs:20-68; defaults there) and the camera terms
 * the path reads (AO.cs:561-573). */
typedef struct meao_params {
    uint32_t struct_size;
    float noise_filter_tolerance;   /* [-8, 0]   default  0     AO.cs:20 */
    float blur_tolerance;           /* [-8,-1]   default -4.6   AO.cs:28 */
    float upsample_tolerance;       /* [-12,-1]  default -12    AO.cs:36 */
    float thickness_modifier;       /* [1, 10]   default  1     AO.cs:44 */
    float intensity;                /* [0, 2]    default  1     AO.cs:52 */
    float near_clip, far_clip;      /* camera.nearClipPlane / farClipPlane  AO.cs:563 */
    float proj00;                   /* camera.projectionMatrix[0,0]         AO.cs:572 */
    int32_t reversed_z;             /* SystemInfo.usesReversedZBuffer       AO.cs:564 */
    int32_t single_pass_stereo;     /* singlePassStereoEnabled (AO.cs:392-401): the frame is the double-wide
                                     * eye pair (cfg.width = 2 * camera.pixelWidth, AO.cs:339,502) and
                                     * ThicknessMultiplier doubles (AO.cs:680) */
} meao_params;

/* Description of one of the 17 debug-visible buffers (AO.cs:789-808). */
typedef struct meao_desc {
    int32_t debug_id;       /* 1..17, or 18..21 = OcclusionHQ1..4 */
    int32_t width, height;
    int32_t slices;         /* 16 for TiledDepth1..4 (AO.cs:154), else 1 */
    int32_t format;         /* meao_format */
    uint64_t bytes;         /* width*height*slices*element size */
} meao_desc;

/* Constant buffers exactly as the reference uploads them. */
typedef struct meao_render_constants {   /* CB1 of Render.compute:38-44, AO.cs:687-734 */
    float inv_thickness_table[12];
    float sample_weight_table[12];
    float inv_slice_dimension[2];
    float reject_fadeoff;
    float intensity;
} meao_render_constants;

typedef struct meao_upsample_constants { /* CB1 of Upsample.compute:41-48, AO.cs:760-771 */
    float inv_low_resolution[2];
    float inv_high_resolution[2];
    float noise_filter_strength;
    float step_size;
    float blur_tolerance;
    float upsample_tolerance;
} meao_upsample_constants;

/* ---- library ------------------------------------------------------------------------ */
MEAO_API int32_t meao_abi_version(void);
MEAO_API const char *meao_status_string(int32_t status);
/* Fills the reference defaults (4 levels, R8, RTZ, strict, batch 1; AO.cs:20-68). */
MEAO_API void meao_default_config(meao_config *cfg);
MEAO_API void meao_default_params(meao_params *p);

/* ---- host-side plan: pure CPU, usable without a GPU ------------------------------------ */
/* RTHandle.CalculateDimensions (AO.cs:276-281): ceil(W / 2^level), level 0..6. */
MEAO_API int32_t meao_level_dims(int32_t width, int32_t height, int32_t level,
                                 int32_t *out_w, int32_t *out_h);
/* CalculateZBufferParams (AO.cs:561-568). */
MEAO_API int32_t meao_zbuffer_params(const meao_params *p, float out[4]);
/* PushRenderCommands constant math (AO.cs:660-734) for level 1..4. */
MEAO_API int32_t meao_render_constants_for(int32_t width, int32_t height, const meao_params *p,
                                           int32_t level, meao_render_constants *out);
/* The same for the variants: source_tiled = 0 -> the source is the non-tiled LowDepth<level>
 * (the !source.isTiled branch, AO.cs:679); sample_set = meao_sample_set. */
MEAO_API int32_t meao_render_constants_variant(int32_t width, int32_t height, const meao_params *p,
                                               int32_t level, int32_t source_tiled, int32_t sample_set,
                                               meao_render_constants *out);
/* PushUpsampleCommands constant math (AO.cs:750-771); low_level 1..4 is the mip of LoResDB. */
MEAO_API int32_t meao_upsample_constants_for(int32_t width, int32_t height, const meao_params *p,
                                             int32_t low_level, meao_upsample_constants *out);
/* Buffer table (AO.cs:453-475): dims/format/bytes of debug buffer 1..17 (and 18..21, OcclusionHQ1..4). */
MEAO_API int32_t meao_describe_buffer(const meao_config *cfg, int32_t debug_id, meao_desc *out);
/* Compulsory traffic of each pass in the reference's storage formats (SURVEY.md 8d,
 * BASELINE.md 3): the numerator of the roofline fraction.  bytes[MEAO_NUM_PASSES]. */
MEAO_API int32_t meao_algorithmic_bytes(const meao_config *cfg, uint64_t bytes[MEAO_NUM_PASSES]);

/* ---- context (replaces DoLazyInitialization / OnDestroy, AO.cs:440-494,357-381) --------- */
MEAO_API int32_t meao_create(const meao_config *cfg, meao_ctx **out_ctx);
MEAO_API int32_t meao_destroy(meao_ctx *ctx);
/* Screen-size change (AO.cs:338-341,501): re-plans and re-allocates the intermediates. */
MEAO_API int32_t meao_resize(meao_ctx *ctx, int32_t width, int32_t height);
/* Dynamic resolution: reserve a maximum size once, then resize without allocating.  (The ABI version is unchanged: hosts probe
 * for these symbols.)
 * meao_reserve sizes the context's intermediates for max_width x max_height -- the arena for max_batch slots, with the second
 * downsample set where the context has one.  It may allocate and synchronises the device once, like meao_resize; it changes no
 * result.  The reservation must cover the current size in both dimensions (else MEAO_ERR_INVALID_ARGUMENT); (0, 0) drops it and
 * returns the context to the exact fit.  On success a ready prefetched set and an announcement are dropped (the buffers moved)
 * and the debug state of the last call is gone as after a resize -- also when the reservation asked for is the one it has;
 * on failure the context is exactly as it was: geometry, buffers, reservation, a ready prefetch; a waiting composite batch stays
 * waiting either way.  meao_get_capacity reports the reservation, (0, 0) = none.  meao_reserve_bytes is host-plan only, like
 * meao_describe_buffer (cfg.width / height are validated but not used): the device memory a reservation of that size costs,
 * max_batch slots with one (cfg.pipelined = 0) or two downsample sets, so that a host can budget before it reserves.
 * Under a reservation every buffer of a slot sits at the offset the RESERVED geometry gives it, and the two downsample sets
 * lie that geometry's set size apart; a buffer is packed for the extents of the current size, which fit because every level's
 * ceil(w / 2^k) x ceil(h / 2^k) is monotone in w and in h.
 * meao_resize to a size inside the reservation (both dimensions) moves nothing: no HIP allocation, no device, stream or event
 * synchronisation, no launch -- except that a waiting composite batch is run as plain launches at the old size on its own
 * stream, as in every resize, which is asynchronous.  It re-plans, and the debug state of the last call is gone, as in every
 * resize.  It can be called in a free-running stream.  Ordering on the device is the rule that already holds between any two
 * executes of one context: they share the intermediates, the stream orders them, and a host that changes streams between
 * calls orders them itself.
 * meao_resize outside the reservation behaves as without one -- it synchronises and allocates, and on failure nothing changes --
 * and the reservation grows to the component-wise maximum of the old reservation and the new size.  On a context that was never
 * given a reservation meao_resize is unchanged in every respect. */
MEAO_API int32_t meao_reserve(meao_ctx *ctx, int32_t max_width, int32_t max_height);
MEAO_API int32_t meao_get_capacity(const meao_ctx *ctx, int32_t *out_width, int32_t *out_height);
MEAO_API int32_t meao_reserve_bytes(const meao_config *cfg, int32_t max_width, int32_t max_height, uint64_t *out_bytes);
/* Property change (AO.cs:104-113): recomputes the per-level constant blocks. */
MEAO_API int32_t meao_set_params(meao_ctx *ctx, const meao_params *p);
MEAO_API int32_t meao_get_params(const meao_ctx *ctx, meao_params *out);
MEAO_API int32_t meao_get_config(const meao_ctx *ctx, meao_config *out);
/* Last error text of this context ("" if none).  Never NULL; ctx may be NULL. */
MEAO_API const char *meao_last_error(const meao_ctx *ctx);

/* ---- the hot path (replaces the recorded "SSAO" CommandBuffer, AO.cs:496-531) ----------- */
/* depth: width*height raw device depth texels in cfg.depth_format (default float32), row-major,
 *        tightly packed (row-pitched surfaces: meao_execute_batch_pitched)
 *        (_CameraDepthTexture / ResolvedDepth, AO.cs:608-641).
 * ao_out: width*height AO texels in cfg.ao_format (the "AmbientOcclusion" RT, AO.cs:475).
 * Alignment of DEVICE pointers: none required.  When width % 4 == 0 and every depth pointer is
 *        aligned to 4 texels (16 bytes for F32 / UNORM24, 8 for the 16-bit formats) the last pass
 *        reads the depth frame with 4-texel vector loads (the downsample pass: width % 8 == 0), and when
 *        every ao_out pointer is also aligned to 4 texels (4 bytes R8, 8 bytes F16) it uses 4-texel stores;
 *        otherwise the scalar variants run (same results, slower).  hipMalloc / torch allocations are
 *        always aligned.
 * The depth frames are read by the FIRST and the LAST pass of the call (the downsample pass builds the four
 *        levels from their even rows; the full-resolution upsample linearizes every texel itself instead of
 *        reading it back from a LinearDepth buffer): they must stay unchanged until the call has completed.
 * Failure: meao_resize and the first meao_prefetch_batch allocate; when that fails the context is left
 *        exactly as it was (geometry, buffers, a ready prefetch).
 * Any depth value is accepted: NaN, +-inf, negative, > 1 or denormal raw depths are processed with
 *        IEEE division exactly like the reference's Linearize (Downsample1.compute:37-48) -- a frame
 *        containing such texels takes slower kernel bodies, results stay bit-exact vs the oracle.
 * *_loc: meao_mem; HOST pointers are staged through context-owned device buffers.
 * Asynchronous on `stream` for DEVICE/DEVICE; returns after completion if either is HOST. */
MEAO_API int32_t meao_execute(meao_ctx *ctx, const void *depth, int32_t depth_loc,
                              void *ao_out, int32_t out_loc, meao_stream stream);
/* n independent frames (n <= cfg.max_batch) through one launch per pass. */
MEAO_API int32_t meao_execute_batch(meao_ctx *ctx, int32_t n, const void *const *depth,
                                    int32_t depth_loc, void *const *ao_out, int32_t out_loc,
                                    meao_stream stream);
/* Pipelining for streams of frames.  Announces the DEVICE depth frames of the call after next: the
 * following meao_execute* carries their downsample pass inside its last upsample kernel (f32 depth,
 * width % 8 == 0, aligned frames; otherwise as one more launch behind it), where the pass's HBM traffic
 * overlaps arithmetic instead of costing a launch between two VALU-bound ones;
 * the meao_execute* after that, if given exactly these n pointers, skips its own downsample pass.
 * Results are identical.  Rules: the announced buffers must hold their final contents before the
 * carrying execute is submitted and stay unchanged until the consuming one has run.  Enforced, not
 * only documented: the prefetched downsample is used only by an execute on the SAME stream as the
 * one that carried it (stream order is what orders the two) and given exactly the announced
 * pointers; any other execute, meao_set_params and meao_resize simply run / re-run the pass.
 * With cfg.pipelined = 1 this call never allocates or synchronises; otherwise the first call
 * re-allocates the context's intermediates with a second set of downsample buffers (one device
 * synchronisation; on allocation failure the context is left unchanged and usable). */
MEAO_API int32_t meao_prefetch_batch(meao_ctx *ctx, int32_t n, const void *const *depth);
/* Per-frame parameters (several cameras in one batch).  meao_execute_batch where frame f uses params[f] instead of the context's
 * parameters.  The context's own parameters (meao_set_params) are neither read nor changed.  Every params[f] is validated like
 * meao_set_params; if any is invalid, nothing is launched and MEAO_ERR_INVALID_ARGUMENT names the frame.  Same launch structure,
 * same contracts (no allocation and no host synchronisation for DEVICE/DEVICE, asynchronous on `stream`); each kernel reads
 * its frame's constants from a context-owned table filled by one copy on `stream`.  The tables form a ring of 8 slots
 * (meao_create allocates it: 8 x max_batch x ~6 KB of device memory and as much pinned host memory): a per-frame call made
 * while the per-frame call 8 calls before it has not yet completed on the device waits for that call first (back-pressure;
 * a host that stays fewer than 8 per-frame calls ahead of the device never waits).  "A per-frame call" is every call that reads
 * its constants from such a table: one given params[], and also a meao_execute_batch that carries an announcement made with
 * params[] (meao_prefetch_batch_params). */
MEAO_API int32_t meao_execute_batch_params(meao_ctx *ctx, int32_t n, const void *const *depth, int32_t depth_loc,
                                           void *const *ao_out, int32_t out_loc, const meao_params *params,
                                           meao_stream stream);
/* meao_prefetch_batch whose frames' downsample pass uses params[f].  A prefetched downsample is reused only if the consuming
 * execute gets the same pointers AND each frame has the same near_clip, far_clip and reversed_z it was computed with
 * (whichever entry point announced or consumes it); otherwise the pass is re-run. */
MEAO_API int32_t meao_prefetch_batch_params(meao_ctx *ctx, int32_t n, const void *const *depth, const meao_params *params);
/* Row-pitched surfaces (linear textures with a row pitch, a viewport inside a larger target, a cropped tensor).
 * depth_pitch / ao_pitch: bytes between the starts of consecutive rows; 0 = tightly packed.  One pitch per surface kind per call;
 * the per-frame pointers already give every frame its own origin.  params: NULL = the context's parameters (meao_execute_batch),
 * else one per frame (meao_execute_batch_params).  Otherwise the contracts of meao_execute_batch / meao_execute_batch_params hold
 * unchanged: no allocation and no host synchronisation for DEVICE/DEVICE, asynchronous on `stream`, the per-frame table ring.
 * Validation, before anything is enqueued (nothing is launched on failure; meao_last_error names the argument):
 *   MEAO_ERR_INVALID_ARGUMENT  a non-zero pitch smaller than width x element size, or not a multiple of the element size
 *                              (depth: 4 F32 / 2 UNORM16 / 4 UNORM24 / 2 F16 bytes; AO: 1 R8 / 2 F16 bytes);
 *   MEAO_ERR_UNSUPPORTED       pitch / element size >= 2^24, or (height - 1) x pitch + width x element size > 2^32 - 1
 *                              (offsets into caller memory are 32-bit byte offsets).
 * DEVICE frames are read and written in place -- no copy, no pack kernel -- by the pitched forms of the kernels that address
 * caller memory (the downsample pass and the full-resolution upsample); pitches of 0 or of the packed row launch exactly the
 * kernels of meao_execute_batch.  The 4-texel vector forms need, beyond the alignment rules of meao_execute_batch, a pitch that
 * is a multiple of 4 texels; otherwise the scalar forms run (same results).  HOST frames are staged packed (hipMemcpy2DAsync), the
 * results copied back into the pitched rows; bytes of a surface outside its width x height texels are never read or written.
 * Pipelining: a prefetched downsample is reused only by a call with the same pointers, the same depth pitch (0 and the packed
 * row count as the same) and the near / far / reversed_z rule of meao_prefetch_batch_params.  Debug ids 1 and 17
 * (meao_get_intermediate, meao_debug_view) honour the last call's pitches.  The composite has pitched forms of its own
 * (meao_composite_pitched); meao_pool_gather_to_device takes tightly packed surfaces only. */
MEAO_API int32_t meao_execute_batch_pitched(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch, int32_t depth_loc,
                                            void *const *ao_out, uint64_t ao_pitch, int32_t out_loc, const meao_params *params,
                                            meao_stream stream);
MEAO_API int32_t meao_prefetch_batch_pitched(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                             const meao_params *params);
/* Announcements that survive a size change (dynamic resolution).  meao_prefetch_batch_pitched for frames of width x height, a size
 * inside the reservation (meao_reserve) that need not be the context's: otherwise MEAO_ERR_INVALID_ARGUMENT, and meao_last_error
 * names the argument; depth_pitch is validated against the ANNOUNCED size; params may be NULL.  The next meao_execute*, at the
 * current size, runs the announced frames' downsample pass at the announced size into the other downsample set: inside its last
 * kernel where the carried form is eligible (f32 depth, width % 8 == 0, aligned frames -- of the announced frames) and the pass's
 * tiles fit that kernel's grid (ceil(w / 128) x ceil(h / 32) announced against ceil(W / 64) x ceil(H / 64) current tiles), else
 * as one more launch behind it; host code decides, no kernel knows.  meao_resize(width, height) KEEPS an announcement or a ready
 * set made by this call for exactly the new size and drops any other -- also every one made by the other meao_prefetch_batch*
 * calls, as ever.  What it keeps is from then on an ordinary announcement or ready set of the context's size: the next resize,
 * also one to the same size, drops it.  The consuming execute matches on the size as well (where the sizes differ the pitches
 * are not compared): a host that announces one size and executes at another gets a correct result from a pass of its own.
 * With width x height equal to the current size the call IS meao_prefetch_batch_pitched.  The frame loop of a host that scales
 * its resolution:
 *   meao_prefetch_batch_sized(B, frames k+1) -> meao_execute*(frames k, at A) -> meao_resize(B) -> meao_execute*(frames k+1)
 * never leaves the pipelined form. */
MEAO_API int32_t meao_prefetch_batch_sized(meao_ctx *ctx, int32_t width, int32_t height, int32_t n, const void *const *depth,
                                           uint64_t depth_pitch, const meao_params *params);
/* Mixed-size batches: one size per frame inside the context's capacity (a 4K main view plus a handful of 256 x 256 probes in
 * one batched launch sequence).  DEVICE surfaces only.  extents[f] gives frame f its own width, height and row pitches (bytes;
 * 0 = tightly packed for THAT frame's width).  The capacity is the reservation (meao_reserve) where the context holds one, else
 * the context's size; every frame needs 1 <= width <= capacity width and 1 <= height <= capacity height, which suffices because
 * ceil(w / 2^k) is monotone (the argument meao_reserve makes for resizes): frame f's intermediates are packed for its own
 * extents inside slot f.  Frame f's AO and every intermediate are bit for bit what a context of size extents[f] gives for that
 * frame with params[f] (NULL: the context's parameters), in every configuration a context can have.  The context's size,
 * parameters and reservation are neither read for the results nor changed.
 * Validation, before anything is enqueued (a refused call launches nothing and leaves an announcement, a ready set and a waiting
 * composite as they were; meao_last_error names the call, the frame and the argument): n, the pointers and params[] as in
 * meao_execute_batch_params; MEAO_ERR_INVALID_ARGUMENT for a size outside the capacity or outside [1, 32768]; each pitch by the
 * rules of meao_execute_batch_pitched against its own frame's size.
 * When every extent equals the context's size and all frames share their pitches the call IS meao_execute_batch_pitched.  Every
 * other call is a "mixed call", a per-frame call (it reads its argument blocks from the table ring) also with params == NULL,
 * under the contracts of meao_execute_batch_params -- no allocation, no host synchronisation, asynchronous on `stream`, the ring
 * of 8 tables -- and: a waiting composite batch is run first as plain launches; a ready prefetched set is consumed unmatched (the
 * call runs its own downsample pass); an announcement (meao_prefetch_batch*, sized or not) is carried as a launch of its own
 * behind the last kernel and promoted as usual (there is no announcement form for mixed batches).  Launch shapes are chosen for
 * the call as a whole: the tile-count thresholds compare the sum over the frames, the 4-texel vector forms need every frame
 * eligible by its own width, pitches and pointers, and each launch has the grid of its largest frame -- workgroups beyond a
 * smaller frame's own tile count return at once.  Afterwards meao_get_intermediate / meao_debug_view (dst / out not NULL)
 * describe and return frame f's buffers at frame f's size; a frame index >= n is refused (MEAO_ERR_INVALID_ARGUMENT), as after
 * every call, and meao_reserve, meao_resize and a re-allocation take the per-frame sizes away with everything else "as left by
 * the last execute".
 * What the rules above imply, spelt out (tests/call_model.py models exactly this):
 *   - "all frames share their pitches" compares row strides in texels: 0 and the packed row in bytes are the same stride.  A call
 *     whose frames all have the context's size but two different strides is a mixed call.
 *   - A mixed call chooses exact division as every per-frame call does: for the call, and only if every frame's parameters
 *     (params[f], or the context's) are inside the exact range.  The ready set it promotes is stamped with that choice.
 *   - meao_hostile_frames afterwards has one bit per frame, in frame order, as after every call.
 *   - The ready set is consumed unmatched also when every component of its key would have matched this call (same pointers, n,
 *     stream, strides, Z-buffer parameters): the key is not compared.
 *   - The ready set a mixed call promotes is an ordinary one: it has the announcement's size if that was sized, else the
 *     context's; its stride; this call's stream; it is matched, kept by meao_resize or dropped by meao_set_params like any other.
 *   - The AO surfaces a mixed call wrote may be named by a later meao_composite_enqueue*, which reads them as it reads every AO
 *     surface: at the CONTEXT's size under the pitch it is given.  Only frames of that size are meaningful input to it.  Frames
 *     of their own sizes are composited by meao_composite_batch_extents, or shaded in the same call by
 *     meao_execute_batch_extents_shaded (below, with the composite calls); there is no enqueued or carried form for them. */
typedef struct meao_extent {
    int32_t width, height;
    uint64_t depth_pitch, ao_pitch;
} meao_extent;
MEAO_API int32_t meao_execute_batch_extents(meao_ctx *ctx, int32_t n, const void *const *depth, void *const *ao_out,
                                            const meao_extent *extents, const meao_params *params, meao_stream stream);
/* Waits for `stream`; NULL = the stream of the last meao_execute* of this context.  meao_composite /
 * meao_composite_flush do not change what NULL means: a composite issued on another stream is waited for
 * by naming that stream here (or by synchronising it directly). */
MEAO_API int32_t meao_synchronize(meao_ctx *ctx, meao_stream stream);

/* ---- observability (replaces the _debug 1..17 views, AO.cs:787-820) --------------------- */
/* Copies debug buffer `debug_id` of batch slot `frame` (as left by the last execute) to dst
 * in the reference's layout (TiledDepth: [16][h][w]).  dst may be NULL to query desc only.
 * Ids 18..21 (OcclusionHQ<k>) exist only for the levels cfg.hq_levels enables.
 * Ids 1 (LinearDepth) and 6..9 (TiledDepth<k>) are not buffers of the hot path: they are built here, on demand, bit-identical
 * to what Downsample1 / Downsample2 would have stored -- id 1 from the DEPTH FRAME the last execute was given, which must
 * therefore still be alive and unchanged (HOST frames are staged by the context and always are). */
MEAO_API int32_t meao_get_intermediate(meao_ctx *ctx, int32_t frame, int32_t debug_id,
                                       void *dst, uint64_t dst_capacity, int32_t dst_loc,
                                       meao_desc *out_desc);

/* The picture the reference's _debug = 1..17 mode shows (PushDebugBlitCommands AO.cs:787-820): the
 * chosen buffer blitted into the full-resolution AO target -- point-sampled at the destination
 * texel centres for the 2D buffers (cmd.Blit(rt, _result)), the 4x4 grid of slices for the tiled
 * arrays (Blit.shader:136-155 pass 4), the result itself for 17.  Sampling positions are evaluated
 * in exact integer arithmetic: source texel = floor((2x+1) * ws / (2W)); the store converts to
 * cfg.ao_format like every AO store.  out: width*height AO texels. */
MEAO_API int32_t meao_debug_view(meao_ctx *ctx, int32_t frame, int32_t debug_id, void *out,
                                 int32_t out_loc, meao_stream stream);

/* ---- composite: the consumer of the AO texture (PushCompositeCommands AO.cs:822-839) ----
 * The reference composites with raster blits (Blit.shader passes 1-3) into the HDR camera target
 * (ARGBHalf) and, in deferred ambient-only mode, GBuffer0 (ARGB32).  Canonical reading of the
 * fixed-function blend: operands widened to f32, one f32 multiply, result rounded to the target
 * format (f16: round-to-nearest-even, the output-merger rule; UNORM8: as the AO stores).
 *   MULTIPLY      pass 2, "Blend Zero SrcAlpha":            color.rgba *= ao
 *   AMBIENT_ONLY  pass 1, "Blend Zero OneMinusSrcColor, Zero OneMinusSrcAlpha", occ = 1 - ao:
 *                 color.rgb *= (1 - occ), color.a unchanged; gbuffer0.a *= (1 - occ), rgb unchanged
 *   DEBUG         pass 3, no blend:                         color.rgba = ao
 * ao: width*height texels in cfg.ao_format; color: width*height RGBA16F (8 bytes per texel),
 * updated in place; gbuffer0: width*height RGBA8, only for AMBIENT_ONLY (else NULL).
 * All pointers share one location `loc`. */
typedef enum meao_composite_mode {
    MEAO_COMPOSITE_MULTIPLY = 0, MEAO_COMPOSITE_AMBIENT_ONLY = 1, MEAO_COMPOSITE_DEBUG = 2
} meao_composite_mode;
MEAO_API int32_t meao_composite(meao_ctx *ctx, int32_t mode, const void *ao, void *color_rgba16f,
                                void *gbuffer0_rgba8, int32_t loc, meao_stream stream);

/* Pipelined composite ("depth in -> shaded frame out" for streams of frames).  The composite moves 17
 * bytes per texel -- as many bytes as the whole AO path -- while the render pass is VALU-bound with
 * HBM nearly idle.  meao_composite_enqueue registers the composite of n DEVICE frames (ao[f] produced
 * by an earlier meao_execute*; same formats and modes as meao_composite); the NEXT meao_execute* on
 * this context carries it inside its render kernel (every render workgroup first streams its share of
 * the texel pairs), on that call's stream, i.e. ordered behind the kernels that wrote ao[f] when the
 * same stream is used.  (A per-frame call -- see meao_execute_batch_params -- and a context with MEAO_SAMPLES_EXHAUSTIVE carry
 * nothing in their render kernels: they run the waiting batch first, as plain launches on the call's stream.)
 * Results are identical to meao_composite.  One batch can wait at a time: a
 * second enqueue, meao_resize and meao_composite_flush run the waiting batch as plain composite
 * launches, on the stream of the execute that preceded its enqueue -- i.e. the one that produced
 * ao[f] -- or on the stream given to meao_composite_flush.  meao_destroy DISCARDS a batch that still
 * waits (its targets are caller memory that is usually gone by then): call meao_composite_flush
 * before destroying a context if the last enqueued composite matters.
 * ao[f], color[f] and gbuffer0[f] must stay valid and untouched until the carrying call has run. */
MEAO_API int32_t meao_composite_enqueue(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao,
                                        void *const *color_rgba16f, void *const *gbuffer0_rgba8);
MEAO_API int32_t meao_composite_flush(meao_ctx *ctx, meao_stream stream);
/* *out_frames = frames of an enqueued composite batch that no execute / flush / resize / second enqueue has run yet
 * (0 = nothing waits).  Hosts ask the library instead of mirroring this state (a batch rides only in the members / calls
 * that actually execute; an execute that fails leaves it waiting). */
MEAO_API int32_t meao_composite_pending(const meao_ctx *ctx, int32_t *out_frames);
/* The composite into row-pitched surfaces (render targets with a row pitch, a viewport inside a larger target, a cropped tensor):
 * meao_composite / meao_composite_enqueue with ao_pitch / color_pitch / gbuffer0_pitch, the bytes between the starts of consecutive
 * rows of the AO, RGBA16F and RGBA8 surfaces; 0 = tightly packed.  One pitch per surface kind per call; the per-frame pointers
 * give every frame its own origin.  gbuffer0_pitch is ignored where gbuffer0 is NULL.  Pitches of 0 or of the packed row run
 * exactly the code of meao_composite / meao_composite_enqueue, which are the pitch-0 forms.  (The ABI version is unchanged:
 * hosts probe for these symbols.)
 * Validation, before anything is launched or enqueued (a refused enqueue leaves a waiting batch waiting, untouched;
 * meao_last_error names the argument):
 *   MEAO_ERR_INVALID_ARGUMENT  a non-zero pitch smaller than width x element size, or not a multiple of the element size
 *                              (AO: 1 R8 / 2 F16 bytes; colour: 8; GBuffer0: 4);
 *   MEAO_ERR_UNSUPPORTED       pitch / element size >= 2^24, or (height - 1) x pitch + width x element size > 2^32 - 1
 *                              (offsets into caller memory are 32-bit byte offsets).
 * DEVICE surfaces are used in place by the kernels that composite packed surfaces (a kernel-uniform branch, no other kernel, no
 * pack copy); bytes of a surface outside its width x height texels are never read or written.  A row has ceil(width / 2) texel
 * pairs (pairs do not run across row ends).  No alignment is required.  The vector form (16-byte colour accesses, two AO texels
 * per load) runs where the colour base and pitch are multiples of 16 bytes and the AO base and pitch multiples of two AO texels --
 * for an enqueued batch, where that holds for every frame; otherwise a per-texel scalar form runs, with the same results.
 * HOST `loc` (meao_composite_pitched only, as for meao_composite) stages the surfaces packed (hipMemcpy2DAsync) and copies the
 * results back into the pitched rows.  A waiting batch remembers its pitches: carried by the next execute's render kernel, run
 * by meao_composite_flush, a second enqueue or meao_resize, or flushed first by a per-frame call or an EXHAUSTIVE context, it
 * composites into the same texels.  The carrying kernel takes the vector-eligible full pairs of a MULTIPLY batch with one
 * composite frame per render frame into its texel loop, as for packed surfaces. */
MEAO_API int32_t meao_composite_pitched(meao_ctx *ctx, int32_t mode, const void *ao, uint64_t ao_pitch,
                                        void *color_rgba16f, uint64_t color_pitch, void *gbuffer0_rgba8, uint64_t gbuffer0_pitch,
                                        int32_t loc, meao_stream stream);
MEAO_API int32_t meao_composite_enqueue_pitched(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                                void *const *color_rgba16f, uint64_t color_pitch,
                                                void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch);

/* The composite into colour targets of other formats.  The reference blends into the camera target whatever its format
 * (AO.cs:822-839): ARGB32 on a camera without HDR, RGB111110Float where the graphics tier selects the packed HDR format, ARGBHalf
 * otherwise; torch pipelines hold float32 images.  In a project in linear colour space (the reference's own setting,
 * ProjectSettings.asset: m_ActiveColorSpace 1) the ARGB32 target of a camera without HDR is an sRGB surface: MEAO_COLOR_RGBA8_SRGB. */
typedef enum meao_color_format {
    MEAO_COLOR_RGBA16F = 0,     /* 8 bytes per texel; what meao_composite* take today */
    MEAO_COLOR_RGBA32F = 1,     /* 16 bytes per texel */
    MEAO_COLOR_RGBA8 = 2,       /* 4 bytes per texel, UNORM, alpha in the top byte: RGBA8 and BGRA8 alike (every mode treats
                                   r, g, b the same) */
    MEAO_COLOR_R11G11B10F = 3,  /* 4 bytes per texel: R bits 0-10, G 11-21, B 22-31 (DXGI R11G11B10_FLOAT,
                                   VK B10G11R11_UFLOAT_PACK32, Unity RGB111110Float); no alpha */
    /* 4 is not assigned and never will be: it stays "not a meao_color_format" */
    MEAO_COLOR_RGBA8_SRGB = 5   /* 4 bytes per texel: r, g, b sRGB-encoded UNORM8 in the low three bytes, blended in linear light;
                                   alpha linear UNORM8 in the top byte.  RGBA8_SRGB and BGRA8_SRGB alike.  Libraries older than
                                   the format refuse the value with MEAO_ERR_INVALID_ARGUMENT, which is how a host probes for
                                   support (no ABI version change, no new entry point) */
} meao_color_format;
/* meao_composite_pitched / meao_composite_enqueue_pitched (and, below, meao_pool_composite_enqueue_pitched) with the format of
 * `color` as an argument; pitch 0 = tightly packed.  With MEAO_COLOR_RGBA16F they run exactly the code of the _pitched calls,
 * which are the RGBA16F forms.  (The ABI version is unchanged: hosts probe for these symbols.)  With MEAO_COLOR_RGBA8,
 * sRGB targets are out of scope: that format multiplies the stored codes as they are, and on an sRGB surface that differs from
 * the fixed-function blend in 59 777 of the 65 536 (code, R8 AO) pairs, by up to 73 codes.  An sRGB target is named
 * MEAO_COLOR_RGBA8_SRGB: blending in linear light needs a transfer function, the reference gives no bit-level definition of one,
 * and that format's two tables below are one.
 * Canonical reading, as above: operands widened to f32, ONE f32 multiply per channel (f = ao in MULTIPLY, keep = 1 - (1 - ao) in
 * AMBIENT_ONLY), the result rounded to the target format:
 *                MULTIPLY                          AMBIENT_ONLY                       DEBUG
 *   RGBA32F      rgba = rgba * ao, as computed     rgb = rgb * keep, a untouched      rgba = ao
 *                (a -0 texel stays -0)
 *   RGBA8        c = unorm8(f32(c) * ao)           rgb = unorm8(f32(c) * keep),       rgba = unorm8(ao)
 *                per channel                       a untouched
 *   R11G11B10F   rgb = enc(dec(c) * ao)            rgb = enc(dec(c) * keep)           rgb = enc(ao)
 *   RGBA8_SRGB   rgb = senc(D[c] * ao),            rgb = senc(D[c] * keep),           rgb = senc(ao), a = unorm8(ao)
 *                a = unorm8(f32(a) * ao)           a untouched
 * unorm8 / f32 are the conversions of the AO stores and of GBuffer0.a: saturate with NaN -> 0, x 255 and + 0.5 as two roundings,
 * truncate; code / 255 correctly rounded.  GBuffer0 is RGBA8 in every colour format and touched in AMBIENT_ONLY only.
 * R11G11B10F channels are unsigned small floats with a 5-bit exponent of bias 15 and M mantissa bits (6 for R and G, 5 for B).
 *   dec, exact:  e = 0: m * 2^(-14 - M);  0 < e < 31: (1 + m / 2^M) * 2^(e - 15);  e = 31: m = 0 +inf, else NaN.
 *   enc(x):      NaN of either sign -> e = 31 with every mantissa bit set (0x7FF / 0x3FF); anything with the sign bit set (-0,
 *                negatives, -inf) -> 0; +inf -> e = 31, m = 0; otherwise round to nearest even with gradual underflow, and a
 *                value that rounds past the largest finite code (65024 for M = 6, 64512 for M = 5) becomes +inf.
 * That is the f16 output-merger rule of the RGBA16F stores restated for a format without a sign.  D3D leaves the float11 /
 * float10 rounding to the implementation: like the f16 stores, this is ONE reading of the blend, the one the tests pin.
 * RGBA8_SRGB: what the fixed-function blend does on an sRGB surface -- decode the destination to linear light, multiply,
 * re-encode -- with the ideal conversions of the D3D functional spec written as two tables of f32 words, so that every output bit
 * is defined.  With lin(s) = s / 12.92 for s <= 0.04045 and ((s + 0.055) / 1.055)^2.4 otherwise (IEC 61966-2-1):
 *   D[k], k = 0..255:  the f32 nearest to the real number lin(k / 255) (D3D's sRGB -> float); D[0] = 0, D[255] = 1.
 *   T[k], k = 1..255:  the smallest f32 that is >= lin((k - 0.5) / 255).
 *   senc(x):           the number of k in 1..255 with x >= T[k]: the nearest code in the encoded domain (D3D's "ideal" float ->
 *                      sRGB, inside the spec's 0.6-ULP allowance), monotone.  NaN of either sign -> 0; anything below T[1] (-0,
 *                      negatives, -inf) -> 0; anything >= T[255] (values above 1, +inf) -> 255.
 * Neither table has a near-tie: in 200-bit arithmetic the closest D value is 5.0e-10 (relative) from a rounding boundary and the
 * closest T boundary 2.8e-11 from an f32, so any arithmetic of 100 bits or more reproduces both.  senc(D[k]) = k for every k: a
 * factor of exactly 1 leaves every texel untouched.  The words of D[k] for k = 1, 10, 11, 128, 254 are 0x399f22b4, 0x3b46eb61,
 * 0x3b5b518e, 0x3e5d0a89, 0x3f7db8de; of T[k] for k = 1, 10, 11, 128, 255: 0x391f22b4, 0x3b3cf936, 0x3b50f2d1, 0x3e5b2d9a,
 * 0x3f7edc0e.  SHA-256 of the 256 little-endian words of D: 48a8f05136456237aae2c5349e5f0199a182daa19b7c099eb542058f794b9c5b; of
 * the 255 words of T[1..255]: 0b408a80ff623c35aef23dc30ed2669cc9893ecc3227e21394a963f4e5bb51de; of the 256 x 256 uint8 table
 * senc(D[c] * (a / 255)) indexed [c][a]: c7ccee49d6fa41ef4c5a950ae2d9263efd487244dee3eeef6adbc3091ffb79df.  The library carries
 * both tables (csrc/meao_srgb_tables.inc, written by tools/gen_srgb_tables.py); meao_selftest(ctx, 9) checks its conversions
 * against them.  Alpha is linear and moves as in RGBA8; every check, pitch rule and vector-eligibility rule is RGBA8's.
 * Validation is that of the _pitched forms with colour element sizes of 8 / 16 / 4 / 4 / 4 bytes; an unknown color_format is
 * MEAO_ERR_INVALID_ARGUMENT (meao_last_error names the argument), and a tightly packed frame of more than 2^32 - 1 bytes of colour
 * MEAO_ERR_UNSUPPORTED.  Surfaces are aligned to their own words (RGBA32F and R11G11B10F: 4 bytes), no further.
 * Where it runs: inside the kernels that composite RGBA16F (a kernel-uniform branch).  Vector form: 16 bytes of colour per lane
 * (one RGBA32F texel, four RGBA8 / R11G11B10F / RGBA8_SRGB texels) and their AO in one load, where colour base and pitch are multiples of 16
 * bytes and AO base and pitch multiples of the AO texels a lane takes (1 / 4); the last width mod 4 texels of a row, and every
 * surface that is not eligible, run a per-texel scalar form with the same results.  An enqueued batch in a format other than
 * RGBA16F is never carried by a render kernel: the next meao_execute* runs it first, as plain launches (one per frame) on its
 * stream -- the rule for per-frame calls and EXHAUSTIVE contexts; flush, second enqueue, resize and destroy are as documented. */
MEAO_API int32_t meao_composite_format(meao_ctx *ctx, int32_t mode, const void *ao, uint64_t ao_pitch,
                                       void *color, int32_t color_format, uint64_t color_pitch, void *gbuffer0_rgba8,
                                       uint64_t gbuffer0_pitch, int32_t loc, meao_stream stream);
MEAO_API int32_t meao_composite_enqueue_format(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                               void *const *color, int32_t color_format, uint64_t color_pitch,
                                               void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch);

/* The batch in one launch, and shaded frames from the execute call.  (The ABI version is unchanged: hosts probe for these symbols.)
 * meao_composite_batch: the n frames (1..cfg.max_batch) ao[f] x color[f] are composited by ONE composite_kernel launch on `stream`
 * (NULL = the context's own stream), now: nothing waits afterwards, meao_composite_pending is unchanged, and a batch that waits
 * from an earlier meao_composite_enqueue* is neither run nor disturbed.  Arguments, formats, modes, pitches, validation and results
 * are those of meao_composite_enqueue_format (n is checked against cfg.max_batch).  DEVICE surfaces only.  The frames' origins
 * travel in a context-owned table filled by a copy on `stream`; the vector form runs where every frame's bases and the pitches
 * are eligible (the rule above), else every frame runs the per-texel form, with the same results.
 * meao_execute_batch_shaded: meao_execute_batch_pitched (DEVICE / DEVICE; params NULL or one per frame) followed, on the same
 * stream, by the batched composite of ao_out[f] into color[f]: when the call has completed, the colour targets are shaded.  The
 * execute half IS that call: the same launches (the fused last kernel included), the same handling of an announced batch and of
 * a waiting enqueued batch (carried by this call's render kernel, or run first), the same state for meao_synchronize(ctx, NULL),
 * the debug buffers and the pass times.  Its own composite is one composite_kernel launch behind the last AO kernel -- in any
 * mode, colour format and pitches, with shared or per-frame parameters, in an EXHAUSTIVE context -- and never waits.
 * Validation comes first, for both calls: every check of the execute and of the composite runs before anything is enqueued.  A
 * refused call launches nothing and leaves the AO, the colour, an announced batch and a waiting enqueued batch as they were;
 * meao_last_error names the call and the argument.
 * Surfaces: the colour targets of distinct frames must not overlap, and no AO surface may overlap a colour target; the
 * behaviour is undefined otherwise (not checked). */
MEAO_API int32_t meao_composite_batch(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                      void *const *color, int32_t color_format, uint64_t color_pitch,
                                      void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch, meao_stream stream);
MEAO_API int32_t meao_execute_batch_shaded(meao_ctx *ctx, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                           void *const *ao_out, uint64_t ao_pitch, const meao_params *params,
                                           int32_t mode, void *const *color, int32_t color_format, uint64_t color_pitch,
                                           void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch, meao_stream stream);

/* Shaded frames from mixed-size batches: the batched composite with one size and one set of pitches per frame.  (The ABI version
 * is unchanged: hosts probe for these symbols.)
 * meao_composite_batch_extents: meao_composite_batch where frame f is extents[f].width x extents[f].height texels under
 * extents[f]'s three pitches (bytes, 0 = tightly packed for THAT frame's width).  DEVICE surfaces only; n in 1..cfg.max_batch; the
 * modes, colour formats and GBuffer0 rules of meao_composite_format.  Frame f's colour and GBuffer0 bytes are bit for bit what
 * meao_composite_format on a context of size extents[f] leaves, and bytes outside a frame's width x height texels are neither
 * read nor written.  The composite uses no intermediates, so the capacity does not bound it: every frame needs width and height
 * in [1, 32768], nothing more.  The context's size is neither read for the results nor changed; nothing waits afterwards;
 * meao_composite_pending, a waiting enqueued batch, an announcement and a ready set are untouched.  The n frames run as ONE
 * composite_kernel launch on `stream` (NULL = the context's own stream): each frame's origins, extent, strides and form travel
 * in a 64-byte entry of a context-owned table filled by one copy on `stream`, in a ring of 8 slots of its own (meao_create
 * allocates it: 8 x max_batch x 64 bytes of device memory and as much pinned host memory, next to the 8 x max_batch x 24 bytes
 * of meao_composite_batch's ring; the back-pressure rule of the per-frame table ring applies to each ring by itself).  Every
 * frame is dealt row by row, and the vector form is chosen PER FRAME: a frame whose colour base and pitch are multiples of 16
 * bytes and whose AO base and pitch are multiples of a lane's AO texels takes it whatever its neighbours do, with the same
 * results either way.  The launch has the workgroups of its largest frame; those beyond a smaller frame's rows touch no memory.
 * When every extent equals the context's size and all frames share their three strides the call IS meao_composite_batch with
 * extents[0]'s pitches (strides are compared in texels, 0 equals the packed row, and GBuffer0's stride counts only where GBuffer0
 * is given -- as in meao_execute_batch_extents); a call whose frames all have the context's size but two different strides is
 * the sized launch.
 * meao_execute_batch_extents_shaded: meao_execute_batch_extents followed, on the same stream, by that composite of ao_out[f] (at
 * extents[f].ao_pitch) into color[f] (at color_pitch[f]; GBuffer0 at gbuffer0_pitch[f]).  color_pitch and gbuffer0_pitch hold one
 * entry per frame, NULL = every frame tightly packed; gbuffer0_pitch is ignored where gbuffer0_rgba8 is NULL.  The execute half IS
 * meao_execute_batch_extents: the same classification (uniform = the pitched call, else a mixed call), the same capacity rule, the
 * same treatment of a waiting composite, a ready set and an announcement, the same "last execute" state and per-frame debug
 * sizes.  The composite is one launch behind the last AO kernel and never waits.  Each half classifies itself: a call that is
 * uniform for the execute may be the sized launch for the composite (two colour strides), and the other way round.
 * Validation, for both calls, before anything is enqueued -- for the shaded call both halves' checks; a refused call launches
 * nothing and leaves the AO, the colours, an announcement, a ready set and a waiting batch as they were.  n, the mode, the
 * pointers and the AMBIENT_ONLY / GBuffer0 rule as in meao_composite_batch; an unknown color_format is
 * MEAO_ERR_INVALID_ARGUMENT; a width or height outside [1, 32768] is MEAO_ERR_INVALID_ARGUMENT; each frame's pitches follow the
 * rules of meao_composite_format against ITS OWN width: non-zero and smaller than width x element size, or not a multiple of the
 * element size: MEAO_ERR_INVALID_ARGUMENT; pitch / element size >= 2^24: MEAO_ERR_UNSUPPORTED; (height - 1) x pitch + width x
 * element size > 2^32 - 1: MEAO_ERR_UNSUPPORTED.  In the sized launch a tightly packed frame is rows of pitch = width, addressed
 * with 32-bit byte offsets like any row, so that last limit applies to packed frames too -- RGBA16F included, which
 * meao_composite_batch takes packed at any size.  meao_last_error names the call, extents[f] (for the shaded call color_pitch[f]
 * / gbuffer0_pitch[f]) and the argument; an error of the execute half comes under the shaded call's name.
 * Surfaces: as for meao_composite_batch. */
typedef struct meao_target_extent {            /* 32 bytes: offsets 0, 4, 8, 16, 24 */
    int32_t width, height;
    uint64_t ao_pitch, color_pitch, gbuffer0_pitch;   /* bytes; 0 = tightly packed for THIS frame's width */
} meao_target_extent;
MEAO_API int32_t meao_composite_batch_extents(meao_ctx *ctx, int32_t mode, int32_t n, const void *const *ao, void *const *color,
                                              int32_t color_format, void *const *gbuffer0_rgba8,
                                              const meao_target_extent *extents, meao_stream stream);
MEAO_API int32_t meao_execute_batch_extents_shaded(meao_ctx *ctx, int32_t n, const void *const *depth, void *const *ao_out,
                                                   const meao_extent *extents, const meao_params *params, int32_t mode,
                                                   void *const *color, int32_t color_format, const uint64_t *color_pitch,
                                                   void *const *gbuffer0_rgba8, const uint64_t *gbuffer0_pitch, meao_stream stream);

/* Per-pass device timing: when enabled, meao_execute* brackets every pass with HIP events on
 * the launch stream; meao_get_pass_times averages each pass over the executes that ran it since
 * the last reset (it waits for the stream of the last execute first); *out_samples = executes measured.
 * ms[MEAO_NUM_PASSES]; passes not run report 0.
 * enable: 0 = off; 1 = every execute; N > 1 = every Nth execute (the first one after the call included), the others run
 * without event records.  An event record is a marker packet between two launches; the events are created with
 * hipEventDisableSystemFence (nothing synchronizes with them but hipEventElapsedTime), so a record does not write back and
 * invalidate the caches: eight of them per 4K x 16 step cost 1 - 3 % of the step depending on the box (bench.py
 * `without_pass_events`; with fenced events it was up to 4 %, and the short launches read 2 us longer).  meao_debug_set
 * MEAO_DEBUG_PROFILE_PASS_MASK restricts the records to chosen passes. */
MEAO_API int32_t meao_set_profiling(meao_ctx *ctx, int32_t enable);
MEAO_API int32_t meao_get_pass_times(meao_ctx *ctx, float ms[MEAO_NUM_PASSES], int32_t *out_samples);

/* ---- multi-GPU: a pool of contexts, one per device, called from one host thread ------------------
 * The path shards across independent frames only (the reference keeps no temporal state,
 * AO.cs:291-308): frame f of a batch goes to member f mod G, every member owns a complete context
 * and a stream on its device, there is no data-path exchange (SURVEY.md 8e / DESIGN.md 7).  This is
 * what an in-process host (the C# component) binds; bench.py's one-process-per-GPU launch over
 * torch.distributed / RCCL is the other way to the same partition.
 * devices: num_devices HIP ordinals (repeats allowed: several members on one device), or NULL for
 * 0..num_devices-1 modulo the visible device count.  cfg.device is ignored; cfg.max_batch is per member.
 * A pool, like a context, is used by one caller thread at a time.  Inside, DEVICE batches are enqueued by one worker
 * thread per member (started by the first such batch, joined by meao_pool_destroy): a member's 4-5 launches cost
 * 10-14 us of host time, and eight members fed one after the other cannot keep up with one 4K frame per GPU
 * (tools/pool_enqueue_cost.py).  A member's context is only ever touched by one thread at a time. */
typedef struct meao_pool meao_pool;
MEAO_API int32_t meao_pool_create(const meao_config *cfg, const int32_t *devices, int32_t num_devices,
                                  meao_pool **out_pool);
MEAO_API int32_t meao_pool_destroy(meao_pool *pool);
MEAO_API int32_t meao_pool_size(const meao_pool *pool);
/* Member context (owned by the pool), e.g. for meao_get_intermediate / meao_set_profiling; NULL if out of range. */
MEAO_API meao_ctx *meao_pool_context(meao_pool *pool, int32_t member);
/* HIP ordinal that processes frame `frame` of a batch (= where DEVICE pointers of that frame must live); -1 on error. */
MEAO_API int32_t meao_pool_device_of_frame(const meao_pool *pool, int32_t frame);
MEAO_API const char *meao_pool_last_error(const meao_pool *pool);
/* meao_set_params on every member. */
MEAO_API int32_t meao_pool_set_params(meao_pool *pool, const meao_params *p);
/* Every meao_pool_* call leaves the calling thread's current HIP device as it found it.  If a member
 * fails, the other members have still been given their work (their launches are in flight and complete
 * normally); the call returns the first failing member's status and meao_pool_last_error names it. */
/* n <= max_batch * members frames; frame f runs on member f mod G, each member's share as one batched
 * launch sequence on its own stream.  DEVICE pointers of frame f must be resident on
 * meao_pool_device_of_frame(f); the call is then asynchronous (meao_pool_synchronize).  HOST pointers
 * are staged per member and the call returns after completion. */
MEAO_API int32_t meao_pool_execute_batch(meao_pool *pool, int32_t n, const void *const *depth, int32_t depth_loc,
                                         void *const *ao_out, int32_t out_loc);
/* meao_prefetch_batch for the pool: announces the n DEVICE depth frames of the call after next, dealt to
 * the members exactly like meao_pool_execute_batch deals them (frame f -> member f mod G), so that each
 * member's next execute carries its share of the next batch's downsample pass.  Create the pool with
 * cfg.pipelined = 1 to keep this call free of allocation.
 * "The call after next" is the POOL's.  An announcement replaces the one before it in every member, also in members it deals
 * no frame to (n < members).  A member that a meao_pool_execute_batch* deals no frame to has been passed by that call: it drops
 * the announcement and the ready downsample set it may hold, so nothing announced for one pool call is carried or reused by a
 * later one (that member runs its own downsample pass in its next call). */
MEAO_API int32_t meao_pool_prefetch_batch(meao_pool *pool, int32_t n, const void *const *depth);
/* The per-frame forms for the pool: params[f] goes with frame f to member f mod G. */
MEAO_API int32_t meao_pool_execute_batch_params(meao_pool *pool, int32_t n, const void *const *depth, int32_t depth_loc,
                                                void *const *ao_out, int32_t out_loc, const meao_params *params);
MEAO_API int32_t meao_pool_prefetch_batch_params(meao_pool *pool, int32_t n, const void *const *depth, const meao_params *params);
/* The pitched forms for the pool (meao_execute_batch_pitched): the pitches go to every member, frame f (and params[f], if given) to
 * member f mod G. */
MEAO_API int32_t meao_pool_execute_batch_pitched(meao_pool *pool, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                                 int32_t depth_loc, void *const *ao_out, uint64_t ao_pitch, int32_t out_loc,
                                                 const meao_params *params);
MEAO_API int32_t meao_pool_prefetch_batch_pitched(meao_pool *pool, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                                  const meao_params *params);
/* meao_execute_batch_extents for the pool: frame f, extents[f] and params[f] (if given) go to member f mod G.  Every member's
 * share is validated against that member's capacity before any member enqueues (one share that is refused refuses the call: no
 * member launches and none changes); members dealt nothing do what they do for meao_pool_execute_batch_pitched (they drop the
 * announcement and the ready set they hold).  Each member classifies ITS OWN share: a member whose share is uniform at its size
 * makes the pitched call -- it may reuse a ready set and carry inside its last kernel -- while another member's share is mixed. */
MEAO_API int32_t meao_pool_execute_batch_extents(meao_pool *pool, int32_t n, const void *const *depth, void *const *ao_out,
                                                 const meao_extent *extents, const meao_params *params);
/* Dynamic resolution for the pool.  meao_pool_reserve: meao_reserve member by member; if member k fails, the members before it
 * keep the larger reservation (a reservation changes no result), no member's size changes, and meao_pool_last_error names the
 * member.  meao_pool_resize is for sizes that EVERY member's reservation covers; anything else is MEAO_ERR_INVALID_ARGUMENT,
 * checked for every member before any member is touched.  It waits on the host until each worker has finished enqueuing the jobs
 * it was handed (no device synchronisation) and then resizes every member inside its reservation: no allocation, no
 * synchronisation.  meao_pool_gather_to_device copies frames of the new size afterwards.  meao_pool_prefetch_batch_sized: the sized
 * announcement, dealt frame f -> member f mod G like every pool call; meao_pool_resize keeps or drops it in every member alike. */
MEAO_API int32_t meao_pool_reserve(meao_pool *pool, int32_t max_width, int32_t max_height);
MEAO_API int32_t meao_pool_resize(meao_pool *pool, int32_t width, int32_t height);
MEAO_API int32_t meao_pool_prefetch_batch_sized(meao_pool *pool, int32_t width, int32_t height, int32_t n, const void *const *depth,
                                                uint64_t depth_pitch, const meao_params *params);
/* meao_composite_enqueue / meao_composite_flush for the pool, frames dealt f -> member f mod G: the composite
 * of frame f rides inside the next execute of the member that owns (and produced) it. */
MEAO_API int32_t meao_pool_composite_enqueue(meao_pool *pool, int32_t mode, int32_t n, const void *const *ao,
                                             void *const *color_rgba16f, void *const *gbuffer0_rgba8);
/* meao_composite_enqueue_pitched for the pool: the pitches go to every member, and every member's share is validated before
 * any member enqueues. */
MEAO_API int32_t meao_pool_composite_enqueue_pitched(meao_pool *pool, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                                     void *const *color_rgba16f, uint64_t color_pitch,
                                                     void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch);
/* meao_composite_enqueue_format for the pool, dealt and validated as meao_pool_composite_enqueue_pitched. */
MEAO_API int32_t meao_pool_composite_enqueue_format(meao_pool *pool, int32_t mode, int32_t n, const void *const *ao, uint64_t ao_pitch,
                                                    void *const *color, int32_t color_format, uint64_t color_pitch,
                                                    void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch);
/* meao_execute_batch_shaded for the pool (DEVICE surfaces on the frames' devices): frame f goes to member f mod G; every member's
 * share is validated (both halves) before any member enqueues; each member that is dealt frames runs its execute and ONE batched
 * composite launch on its stream, from its worker thread.  Members dealt nothing do what they do for
 * meao_pool_execute_batch_pitched. */
MEAO_API int32_t meao_pool_execute_batch_shaded(meao_pool *pool, int32_t n, const void *const *depth, uint64_t depth_pitch,
                                                void *const *ao_out, uint64_t ao_pitch, const meao_params *params,
                                                int32_t mode, void *const *color, int32_t color_format, uint64_t color_pitch,
                                                void *const *gbuffer0_rgba8, uint64_t gbuffer0_pitch);
/* meao_execute_batch_extents_shaded for the pool: frame f and all its per-frame arguments (extents[f], params[f], color_pitch[f],
 * gbuffer0_pitch[f]) go to member f mod G.  Every member's share is validated, both halves, against that member's capacity
 * before any member enqueues; one refused share refuses the call, and no member launches or changes.  Each member that is dealt
 * frames runs its execute and ONE composite launch on its stream, from its worker thread, and classifies each half of its own
 * share.  Members dealt nothing do what they do for meao_pool_execute_batch_extents. */
MEAO_API int32_t meao_pool_execute_batch_extents_shaded(meao_pool *pool, int32_t n, const void *const *depth, void *const *ao_out,
                                                        const meao_extent *extents, const meao_params *params, int32_t mode,
                                                        void *const *color, int32_t color_format, const uint64_t *color_pitch,
                                                        void *const *gbuffer0_rgba8, const uint64_t *gbuffer0_pitch);
MEAO_API int32_t meao_pool_composite_flush(meao_pool *pool);
MEAO_API int32_t meao_pool_composite_pending(const meao_pool *pool, int32_t *out_frames);   /* summed over the members */
/* Copies the n DEVICE results ao_src[f] (on their owning devices) to dst[f] on dst_device with
 * hipMemcpyPeerAsync (xGMI), each on its producer's stream, i.e. ordered behind the kernels that wrote it. */
MEAO_API int32_t meao_pool_gather_to_device(meao_pool *pool, int32_t n, const void *const *ao_src,
                                            void *const *dst, int32_t dst_device);
/* How a copy from `member`'s device to dst_device travels.  meao_pool_create asks hipDeviceCanAccessPeer for
 * every ordered pair of distinct member devices and enables peer access both ways where it is offered;
 * PEER_DIRECT = enabled (device-to-device over xGMI), STAGED = not offered or not enabled (the runtime
 * bounces the copy through host memory), SAME_DEVICE = no link involved.  Negative = invalid argument. */
typedef enum meao_pool_path { MEAO_POOL_PATH_SAME_DEVICE = 0, MEAO_POOL_PATH_PEER_DIRECT = 1, MEAO_POOL_PATH_STAGED = 2 } meao_pool_path;
MEAO_API int32_t meao_pool_gather_path(const meao_pool *pool, int32_t member, int32_t dst_device);
MEAO_API int32_t meao_pool_synchronize(meao_pool *pool);
/* Host placement.  The eight GPUs of a node hang off two sockets; the thread that enqueues a GPU's launches should run on the
 * socket the GPU hangs off.  meao_device_numa_node: *out_node = NUMA node of HIP device `device` (sysfs numa_node of its PCI
 * function; -1 = the kernel knows none: single-node hosts, most VMs), cpulist (may be NULL) = that node's CPUs in the kernel's
 * "0-15,32-47" form -- what a one-process-per-GPU host (bench.py --gpus N) binds its rank to.  The pool does the same for its
 * worker threads: each binds itself to the allowed CPUs of its member's node when it starts (MEAO_POOL_BIND_NUMA, default 1; the
 * calling thread's cgroup / taskset mask is respected; nothing happens where no node is known).  MEAO_POOL_SPIN_US: how long a
 * worker spins for its next job before it sleeps on a condition variable (default 100; 0 = sleep at once; a stream of 4K steps
 * posts a job every ~60 us per member).  meao_pool_member_placement reports the member's node and whether its worker is bound. */
typedef enum meao_pool_option { MEAO_POOL_SPIN_US = 0, MEAO_POOL_BIND_NUMA = 1 } meao_pool_option;
MEAO_API int32_t meao_device_numa_node(int32_t device, int32_t *out_node, char *cpulist, uint64_t cpulist_capacity);
MEAO_API int32_t meao_pool_configure(meao_pool *pool, int32_t key, int32_t value);
MEAO_API int32_t meao_pool_member_placement(const meao_pool *pool, int32_t member, int32_t *out_numa_node, int32_t *out_worker_bound);

/* Which frames of the last meao_execute* held "hostile" depth texels (NaN, inf, negative, > 1, denormal --
 * anything outside the operand range the exact v_rcp_f32 division sequences are verified for) and therefore
 * ran the slower IEEE-division kernel bodies: bit f of *out_mask = frame f.  Results are bit-exact either
 * way; this is a performance diagnostic.  Synchronises the stream of that call. */
MEAO_API int32_t meao_hostile_frames(meao_ctx *ctx, uint64_t *out_mask);

/* Launch-structure overrides for tests and A/B runs (the library reads no environment variables).  Every
 * structure gives bit-identical results; the defaults are what measured fastest.  FUSE_COARSE_BLEND 0 = three
 * separate blend launches; *_MAX_TILES = tile-count thresholds at or below which a call uses the nested
 * three-level blend launch / 128x8 render tiles / 64x32 final tiles / one-row-per-lane downsample tiles (0 = never).
 * (ABI 6 retired the keys of launch structures that lost every A/B: DS_SHARE_IN_BLEND, DS_SIDE_STREAM, RENDER_FROM_DEPTH*;
 * their patches are kept under profiles/.  Fault injection lives in the `testhooks` variant library only.) */
typedef enum meao_debug_key {
    MEAO_DEBUG_FUSE_COARSE_BLEND = 0, MEAO_DEBUG_NESTED_MAX_TILES = 1, MEAO_DEBUG_RENDER_SMALL_MAX_TILES = 2,
    MEAO_DEBUG_FINAL_SMALL_MAX_TILES = 3, MEAO_DEBUG_DS_SMALL_MAX_TILES = 4,
    MEAO_DEBUG_BLEND_TALL_MIN_TILES = 5, /* L2 -> L1 blend launches of at least this many 64x32 tiles (frames x tiles) use 64x64 tiles, either AO
                                          * storage format; 0 = never.  Default: 4096, R8 storage only */
    MEAO_DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH = 7, /* 1 = the announced next batch's downsample pass (meao_prefetch_batch) runs as a launch of its own
                                               * behind the last upsample kernel instead of inside it (what frames that do not take the
                                               * carried tile's 16-byte loads get anyway); default 0 */
    MEAO_DEBUG_PROFILE_PASS_MASK = 6     /* meao_set_profiling: bit k set = launch slot k (meao_pass) is bracketed with events; 0 = all (default).
                                          * Each event record is a marker packet between two launches (1 - 4 % of a batched step for all
                                          * eight): a host that wants one kernel's duration in a throughput run asks for that slot only */
} meao_debug_key;
MEAO_API int32_t meao_debug_set(meao_ctx *ctx, int32_t key, int32_t value);

/* roctx ranges ("meao:downsample", "meao:render", "meao:upsample_L1_to_L0", ...) around the launches
 * of every pass, so that rocprofv3 --marker-trace output is self-describing even where passes are
 * fused.  Off by default; librocprofiler-sdk-roctx.so (rocprofv3) or libroctx64.so is loaded on first
 * use (MEAO_ERR_UNSUPPORTED if neither is present). */
MEAO_API int32_t meao_set_tracing(meao_ctx *ctx, int32_t enable);

/* Exhaustive device self-tests of what bit-exactness rests on; *out_mismatches = number of
 * inputs whose hardware result differs from the IEEE / bit-level model.
 * which: 0 = f32->f16 RTZ_CLAMP (all 2^32), 1 = f32->f16 RTNE (all 2^32), 2 = unorm8->f32 (256),
 *        3 = f16->f32 (65536), 4 = exact reciprocal vs 1/x (all x, 2^-100<=|x|<=2^100),
 *        (and: the uncorrected v_rcp_f32 within one ulp of it), 5 = exact 3/x and 9/x (same range), 6 = exact a/b on hashed
 *        pairs (2^-60<=|a|,|b|<=2^60), 7 = the UNORM8 bilateral result that skips the correction steps away from rounding
 *        boundaries vs the code of the exact chain, 2^32 hashed operand sets, 8 = f32->float11 and f32->float10 of the
 *        R11G11B10F stores (meao_color_format; all 2^32 inputs, both mantissa widths), 9 = the conversions of
 *        MEAO_COLOR_RGBA8_SRGB: f32 -> sRGB code as the composite kernels compute it vs a search over the table T (all 2^32
 *        inputs), and code -> f32 vs the table D (256). */
MEAO_API int32_t meao_selftest(meao_ctx *ctx, int32_t which, uint64_t *out_mismatches);

#ifdef __cplusplus
}
#endif
#endif /* MEAO_H */
