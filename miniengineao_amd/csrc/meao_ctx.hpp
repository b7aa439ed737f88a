// meao_ctx.hpp -- the context of the C ABI layer (host only; no kernel unit includes this): struct meao_ctx as named parts
// with one owner each, the error helpers, and what the host units (meao_api / meao_execute / meao_composite / meao_debug /
// meao_pool .cpp) call of each other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "meao_kernels.hpp"
#include "meao_plan.hpp"

#ifndef MEAO_TESTING
#define MEAO_TESTING 0      // 1: the `testhooks` variant library -- exports meao_test_* fault injection, never the product
#endif

namespace meao {

constexpr uint64_t kAlign = 256;
constexpr int kProfileRing = 256;         // executes buffered before timings are folded
constexpr int kProfSlots = MEAO_NUM_PASSES;   // launch slots of one execute: one start / end event pair each
inline uint64_t align_up(uint64_t v) { return (v + kAlign - 1) / kAlign * kAlign; }
inline uint64_t ao_elem(const meao_config &c) { return c.ao_format == MEAO_AO_R8 ? 1 : 2; }
inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int fail(meao_ctx *ctx, int status, const std::string &msg);
int fail_hip(meao_ctx *ctx, hipError_t e, const char *what);
// Every synchronising HIP call a context makes (device, stream, event) is counted: what meao_test_counters reports in the
// `testhooks` variant library (a meao_resize inside a reservation must leave the count alone).
void note_sync(meao_ctx *ctx);

#define MEAO_HIP(ctx, expr)                                              \
    do {                                                                 \
        hipError_t e_ = (expr);                                          \
        if (e_ != hipSuccess) return ::meao::fail_hip((ctx), e_, #expr); \
    } while (0)

// Where the intermediates of one frame live inside its slot; a pure function of (plan, cfg, two_ds_sets).  The plan is that of
// the geometry the slots are laid out for: the context's size, or its reservation (meao_reserve) -- then every size inside the
// reservation uses these offsets, each buffer packed for its own extents (ceil(w / 2^k) * ceil(h / 2^k) is monotone in w and h).
struct SlotLayout {
    // Downsample outputs (LowDepth1..4; LinearDepth is never materialised on the hot path).  With meao_prefetch_batch in use the
    // slot holds two such sets: the passes of a call read set `ds_cur` while its last kernel fills the other one with the next
    // batch's downsample.
    uint64_t off_ds_low[4] = {}, ds_set_bytes = 0;
    uint64_t off_occ[4] = {}, off_comb[3] = {};
    uint64_t off_hq[4] = {};                  // OcclusionHQ<k>: only the levels cfg.hq_levels enables
    uint64_t slot_bytes = 0;
    uint64_t off_low_of(int set, int k) const { return off_ds_low[k] + ds_set_bytes * set; }
};

// Launch structures with identical results, chosen by call size; meao_debug_set overrides the thresholds (tests, A/B runs) --
// the library reads no environment variables.
struct Tuning {
    bool fuse_coarse_blend = true;     // Upsample L4->L3 evaluated inside the L3->L2 launch (upsample_two_level_kernel)
    int ds_small_max_tiles = 640;      // stand-alone downsample pass: calls with at most this many 128x16 (LowDepth1 texels) tiles use 128x8 tiles
    int final_small_max_tiles = 2048;  // plain final pass: calls with at most this many 64x64 tiles (one 4K frame: 2040) use 64x32 tiles (r04 sweep: 60.3 vs 60.8 us)
    int render_small_max_tiles = 256;  // calls with at most this many 128x32 render tiles (frames x tiles) use 128x8 tiles
    int nested_max_tiles = 1024;       // calls with at most this many L2->L1 tiles (frames x tiles; one 4K frame: 1020) run the three blend passes as one launch
                                       // (with the round-4 blend_window_into_lds: 55.9 vs 56.6 us per pipelined 4K frame, a tie unpipelined; 512 before)
    // L2 -> L1 launches of at least this many 64x32 tiles (frames x tiles; 4K: 1020 per frame) use 64x64 tiles with R8 AO storage
    // (upsample_blend_tall_kernel): 53.9 -> 52.5 us per 16 frames at 4K, 57.7 -> 56.3 at 1080p x 64, fp16 storage +-0
    // (profiles/r05_ab_blend_tall.jsonl).  MEAO_DEBUG_BLEND_TALL_MIN_TILES overrides it for both storage formats.
    int blend_tall_min_tiles = 4096;
    bool blend_tall_forced = false;
    // The announced next batch's downsample pass (meao_prefetch_batch) always as a launch of its own behind the last kernel instead of
    // inside it (MEAO_DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH; what calls whose frames do not take the carried tile's 16-byte loads do anyway)
    bool next_ds_own_launch = false;
};

// A batch announced by meao_prefetch_batch, consumed by the next execute (tests/call_model.py Announcement).
struct Announcement {
    int n = 0;
    const void *depth[MEAO_MAX_BATCH] = {};
    int32_t depth_pitch = 0;                      // row stride in texels, the frames' width when tightly packed
    bool per_frame = false;                       // it came with its own parameters (prm, plan)
    meao_params prm[MEAO_MAX_BATCH] = {};
    std::vector<Plan> plan;                       // MEAO_MAX_BATCH, sized by meao_create
    // meao_prefetch_batch_sized: frames of another size than the context's (inside its reservation), and the plan of that size
    // for the context's parameters.  sized = false: the context's size and plan at the time of the carrying call.
    bool sized = false;
    int32_t width = 0, height = 0;
    Plan shared_plan{};
};

// ZBufferParams inputs (near, far, reversed_z) a frame of a ready set was downsampled with
struct ZbInputs { float near_clip, far_clip; int32_t reversed_z; };

// A downsample set already filled from exactly these frames (tests/call_model.py ReadySet).  It is only valid on the stream of
// the execute that carried it, for frames of the same pitch and Z-buffer inputs, and -- where the consuming call divides
// exactly -- only if the carrying pass stamped the hostile flags.
struct ReadySet {
    int n = 0, set = 0;
    hipStream_t stream = nullptr;
    int32_t depth_pitch = 0;
    bool sized = false;                           // it came from a sized announcement: a meao_resize to its size keeps it
    int32_t width = 0, height = 0;                // the size its levels were built for
    const void *depth[MEAO_MAX_BATCH] = {};
    ZbInputs zb[MEAO_MAX_BATCH] = {};
    bool exact = false;
};

// The prefetch state machine: announce -> (carried by an execute) promote -> ready -> (matched by an execute) consumed.
// Nothing outside these functions writes its fields.
struct Prefetch {
    Announcement next;
    ReadySet ready;
    int ds_cur = 0;                               // the set the current / last call's passes read
    // generations of the hostile-depth flags (meao_dev_downsample.hpp nice_denominator): a pass stamps its set's words with its
    // generation, so direct launches take a fresh one per pass instead of clearing flags.  Never 0.
    uint32_t gen_counter = 0, set_gen[2] = {0, 0};

    int other() const { return 1 - ds_cur; }
    uint32_t generation() const { return set_gen[ds_cur]; }

    // width x height: the announced frames' size; sized (meao_prefetch_batch_sized): it is not the context's, and
    // ctx_prm the context's parameters, for the plan of that size
    void announce(const meao_config &cfg, int32_t width, int32_t height, bool sized, const meao_params &ctx_prm, int n,
                  const void *const *depth, int32_t pitch, const meao_params *params)
    {
        next.n = n;
        next.depth_pitch = pitch;
        next.sized = sized; next.width = width; next.height = height;
        if (sized) build_plan(width, height, cfg.num_levels, cfg.sample_set, ctx_prm, &next.shared_plan);
        for (int f = 0; f < n; ++f) next.depth[f] = depth[f];
        next.per_frame = params != nullptr;
        if (params)
            for (int f = 0; f < n; ++f) {
                next.prm[f] = params[f];
                build_plan(width, height, cfg.num_levels, cfg.sample_set, params[f], &next.plan[f]);
            }
    }
    // the announcement goes; ready_too: a ready set as well
    void withdraw(bool ready_too)
    {
        next.n = 0; next.per_frame = false; next.sized = false;
        if (ready_too) { ready.n = 0; ready.stream = nullptr; ready.sized = false; }
    }
    // meao_resize(width, height) inside a reservation: a sized announcement and a ready set made from one, for exactly the new
    // size, stay (the buffers do not move and the parameters do not change); everything else goes, as in every resize.  A kept
    // announcement becomes one for the context's size, like any other the next call carries.
    void resized_to(int32_t width, int32_t height)
    {
        if (!(next.n > 0 && next.sized && next.width == width && next.height == height)) { next.n = 0; next.per_frame = false; }
        next.sized = false;
        if (!(ready.n > 0 && ready.sized && ready.width == width && ready.height == height)) { ready.n = 0; ready.stream = nullptr; }
        ready.sized = false;
    }
    static bool same_zb(const ZbInputs &z, const meao_params &p, int depth_format)
    {
        if (linear_depth(depth_format)) {      // linear view-space depth reads s = RN(1 / far_clip) only
            const float s0 = 1.0f / z.far_clip, s1 = 1.0f / p.far_clip;
            return std::memcmp(&s0, &s1, sizeof(float)) == 0;
        }
        return std::memcmp(&z.near_clip, &p.near_clip, sizeof(float)) == 0 && std::memcmp(&z.far_clip, &p.far_clip, sizeof(float)) == 0 &&
               (z.reversed_z != 0) == (p.reversed_z != 0);
    }
    bool matches(int n, const void *const *depth, hipStream_t stream, int32_t pitch, bool exact, const meao_params *const *prm_of,
                 int depth_format, int32_t width, int32_t height) const
    {
        bool ok = ready.n == n && ready.stream == stream && std::memcmp(ready.depth, depth, sizeof(void *) * n) == 0 &&
                  (ready.exact || !exact) && ready.depth_pitch == pitch && ready.width == width && ready.height == height;
        for (int f = 0; ok && f < n; ++f) ok = same_zb(ready.zb[f], *prm_of[f], depth_format);
        return ok;
    }
    // A call begins: it reads the ready set if that matched, else set 0 under a fresh generation.  The ready set is consumed.
    void begin_call(bool matched)
    {
        ds_cur = matched ? ready.set : 0;
        ready.n = 0;
        if (!matched) set_gen[ds_cur] = fresh_generation();
    }
    uint32_t generation_for_next() { return set_gen[other()] = fresh_generation(); }
    // The call carried the announced pass: the announcement becomes the ready set.  width x height: the context's size, which
    // an announcement that is not sized was made for.
    void promote(hipStream_t stream, bool exact, const meao_params &ctx_prm, int32_t width, int32_t height)
    {
        ready.n = next.n; ready.set = other(); ready.stream = stream; ready.exact = exact; ready.depth_pitch = next.depth_pitch;
        ready.sized = next.sized;
        ready.width = next.sized ? next.width : width; ready.height = next.sized ? next.height : height;
        std::memcpy(ready.depth, next.depth, sizeof ready.depth);
        for (int f = 0; f < next.n; ++f) {
            const meao_params &q = next.per_frame ? next.prm[f] : ctx_prm;
            ready.zb[f] = ZbInputs{q.near_clip, q.far_clip, q.reversed_z != 0};
        }
        withdraw(false);
    }

private:
    uint32_t fresh_generation() { if (++gen_counter == 0) ++gen_counter; return gen_counter; }
};

// A ring of N tables of T (max_batch entries each): a call builds its table in pinned host memory and copies it to the device
// slot on its stream; both are reused once the event recorded behind that call's work has completed.  The host waits only when
// it runs N calls ahead (include/meao.h).
template <typename T, int N>
struct TableRing {
    T *table = nullptr, *stage = nullptr;
    hipEvent_t ev[N] = {};
    bool pending[N] = {};
    int pos = 0, per_slot = 0;

    // A slot in use by one call.  From the moment its copy is queued (arm), whatever the call does next -- all its launches, or
    // an early return on a failed one -- the slot is handed back guarded: an event recorded behind the call's work on its stream
    // (reuse waits for it), or, if even that fails, a synchronised stream.
    struct Lease {
        TableRing *ring = nullptr;
        meao_ctx *ctx = nullptr;
        int slot = 0;
        hipStream_t stream = nullptr;
        bool armed = false;
        Lease() = default;
        Lease(const Lease &) = delete;
        Lease &operator=(const Lease &) = delete;
        T *host() const { return ring->stage + static_cast<size_t>(slot) * ring->per_slot; }
        T *device() const { return ring->table + static_cast<size_t>(slot) * ring->per_slot; }
        void arm() { armed = true; }
        ~Lease()
        {
            if (!armed) return;
            if (hipEventRecord(ring->ev[slot], stream) == hipSuccess) {
                ring->pending[slot] = true;
            } else {
                (void)hipGetLastError();
                note_sync(ctx);
                (void)hipStreamSynchronize(stream);
            }
        }
    };

    hipError_t create(int max_batch)
    {
        per_slot = max_batch;
        const size_t bytes = sizeof(T) * N * max_batch;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&table), bytes);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&stage), bytes, hipHostMallocDefault);
        for (int i = 0; e == hipSuccess && i < N; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return e;
    }
    void destroy()
    {
        if (table) (void)hipFree(table);
        if (stage) (void)hipHostFree(stage);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    // The next slot for a call on `stream`, not yet armed.  Back-pressure only: the slot's previous call is N calls old.
    int acquire(meao_ctx *ctx, hipStream_t stream, Lease *lease)
    {
        const int slot = pos;
        pos = (pos + 1) % N;
        if (pending[slot]) {
            // (a host that stays fewer than N calls ahead finds that call completed and makes no synchronising call at all)
            const hipError_t done = hipEventQuery(ev[slot]);
            if (done == hipErrorNotReady) {
                (void)hipGetLastError();
                note_sync(ctx);
                MEAO_HIP(ctx, hipEventSynchronize(ev[slot]));
            } else if (done != hipSuccess) {
                return fail_hip(ctx, done, "hipEventQuery (per-frame table ring)");
            }
            pending[slot] = false;
        }
        lease->ring = this; lease->ctx = ctx; lease->slot = slot; lease->stream = stream;
        return MEAO_OK;
    }
};

// A grow-only device allocation.
struct DeviceBuffer {
    char *ptr = nullptr;
    uint64_t bytes = 0;
    int reserve(meao_ctx *ctx, uint64_t need, const char *what)
    {
        if (bytes >= need) return MEAO_OK;
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr), need);
        if (e != hipSuccess) return fail_hip(ctx, e, what);
        bytes = need;
        return MEAO_OK;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
};

// What the last execute ran on, for the buffers built on demand afterwards (debug ids 1, 6-9, 17) and the stream-less calls.
struct LastCall {
    int frames = 0;
    hipStream_t stream = nullptr;
    bool mixed = false;                          // a mixed call (meao_execute_batch_extents): every frame has its own size
    struct Frame {
        const void *depth, *out;                 // device addresses of the raw depth frame (debug id 1) and of the result (17)
        float zp[2];                             // the parameters the call used for this frame
        int32_t reversed_z;
        float pad[4];
        int32_t width, height;                   // the frame's size: the context's at the time of the call, or its own (mixed)
        uint64_t depth_pitch, out_pitch;         // of the device frame, in bytes; 0 = packed (debug ids 1 and 17 pack it first)
    } frame[MEAO_MAX_BATCH] = {};
};

// Per-pass timing: a ring of per-execute event sets (one start / end pair per launch slot); each entry remembers which slots it used.
struct Profiler {
    bool on = false;
    uint32_t mask = ~0u;                         // MEAO_DEBUG_PROFILE_PASS_MASK: bit k = launch slot k is bracketed with events
    uint32_t period = 1, phase = 0;              // meao_set_profiling(N > 1): every Nth execute is bracketed with events, the others run bare
    std::vector<hipEvent_t> events;              // kProfileRing * kProfSlots * 2
    int ring_fill = 0;
    uint32_t ran_mask[kProfileRing] = {};        // bit k: launch slot k ran in that execute
    double pass_ms_sum[MEAO_NUM_PASSES] = {};
    int pass_samples[MEAO_NUM_PASSES] = {};      // executes that ran pass k
    int executes_profiled = 0;
    hipEvent_t *cur = nullptr;                   // the event set of the call under way, null = it runs bare
    meao_ctx *owner = nullptr;                   // whose synchronising calls fold() makes (note_sync)

    hipEvent_t *begin_call()
    {
        cur = nullptr;
        if (on) {
            if (phase == 0) {
                if (ring_fill == kProfileRing) fold();
                cur = &events[ring_fill * kProfSlots * 2];
            }
            if (++phase >= period) phase = 0;
        }
        return cur;
    }
    bool bracket(int slot) const { return slot >= 0 && (mask >> slot & 1u); }
    void end_call(uint32_t ran) { if (cur) ran_mask[ring_fill++] = ran; }
    void fold();                                 // meao_api.cpp: waits for the buffered events and adds them to the sums
};

// roctx ranges around every pass (meao_set_tracing); libroctx64.so is loaded on first use
struct Tracer {
    bool on = false;
    void *lib = nullptr;
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
};
struct TraceRange {   // roctx range around one pass (no-op unless meao_set_tracing enabled it)
    const Tracer &t;
    TraceRange(const Tracer &tracer, const char *name) : t(tracer) { if (t.on && t.push) t.push(name); }
    ~TraceRange() { if (t.on && t.pop) t.pop(); }
};

}  // namespace meao

struct meao_ctx {
    meao_config cfg{};
    meao_params prm{};
    meao::Plan plan{};
    // operands of every divide provably inside the exact range of the v_rcp_f32 sequences
    // (meao_dev.hpp "Exact division"); recomputed by update_plan()
    int exact_rcp_div = 0;
    hipStream_t own_stream = nullptr;

    // context-owned intermediates: max_batch identical slots inside one arena
    char *arena = nullptr;
    meao::SlotLayout lay;
    bool two_ds_sets = false;
    // meao_reserve: the size the slots are laid out and the arena is allocated for; (0, 0) = none, they fit cfg exactly.
    // A meao_resize inside it changes cfg and the plan only.
    int32_t cap_w = 0, cap_h = 0;
    bool within_reservation(int32_t w, int32_t h) const { return cap_w > 0 && w <= cap_w && h <= cap_h; }
    // What bounds the frames of a mixed call (meao_execute_batch_extents): the reservation, else the context's size
    bool within_capacity(int32_t w, int32_t h) const { return cap_w > 0 ? (w <= cap_w && h <= cap_h) : (w <= cfg.width && h <= cfg.height); }
    // Hostile-depth flags (meao_dev_downsample.hpp nice_denominator): [set][frame] words the downsample pass
    // stamps with its generation when a frame's levels hold texels outside the exact-division range.
    uint32_t *hostile = nullptr;
    uint32_t *hostile_of(int set) const { return hostile + set * MEAO_MAX_BATCH; }
    template <typename T>
    T *slot_ptr(uint64_t off) const { return reinterpret_cast<T *>(arena + off); }

    meao::Tuning tuning;
    meao::Prefetch prefetch;
    meao::LastCall last;

    // Per-frame parameters (meao_execute_batch_params / meao_prefetch_batch_params): the FrameArgs tables of the calls that read
    // per-frame constants, and the plans of the current call's frames.  The batched composite's CompositeFrame tables
    // (meao_composite_batch / meao_execute_batch_shaded) go through a ring of the same kind.  Both allocated by meao_create.
    meao::TableRing<meao::FrameArgs, 8> frame_ring;
    meao::TableRing<meao::CompositeFrame, 8> comp_ring;
    // ... and the sized composite's 64-byte CompositeSizedFrame tables (meao_composite_batch_extents /
    // meao_execute_batch_extents_shaded) through one of their own, so that the uniform batch's entries stay 24 bytes
    meao::TableRing<meao::CompositeSizedFrame, 8> comp_sized_ring;
    std::vector<meao::Plan> frame_plan;          // MEAO_MAX_BATCH

    // a composite batch waiting to ride inside the next execute's render kernel (meao_composite_enqueue),
    // and the stream its AO frames were produced on (where a flush that is not given a stream runs it)
    meao::CompositeBatchArgs pending_comp{};
    int32_t pending_comp_format = MEAO_COLOR_RGBA16F;     // meao_color_format of its colour surfaces; only an RGBA16F batch is ever carried
    hipStream_t pending_stream = nullptr;

    // lazily allocated: staging for HOST in/out and the debug view, scratch for the buffers built on demand (LinearDepth,
    // TiledDepth<k>), packed copies of the last call's pitched frames (debug ids 1 and 17), selftest counter
    meao::DeviceBuffer stage_depth, stage_out, stage_view, atlas_scratch, pack_scratch;
    unsigned long long *counter = nullptr;

#if MEAO_TESTING
    int debug_fail_allocs = 0;         // meao_test_fail_next_allocs: arena allocations still to fail (testhooks variant only)
#endif
    // meao_test_counters (exported by the testhooks variant only): arena allocations attempted, synchronising HIP calls made
    uint64_t arena_allocs = 0, sync_calls = 0;

    meao::Profiler profiler;
    meao::Tracer tracer;

    std::string err;
};

namespace meao {

// An execute's inputs and outputs as the caller gave them (pitches in bytes, 0 = tightly packed; params null = the context's).
struct FrameSet {
    int32_t n;
    const void *const *depth; uint64_t depth_pitch; int32_t depth_loc;
    void *const *out; uint64_t out_pitch; int32_t out_loc;
    const meao_params *params;
    // meao_execute_batch_extents: frame f's own size and pitches (depth_pitch / out_pitch above are then unused); null = every
    // frame has the context's size
    const meao_extent *extents = nullptr;

    // Member m's frames of a pool of G (frame f -> member f mod G), pointers, parameters and extents, in the caller's `storage`.
    struct Storage { const void *depth[MEAO_MAX_BATCH]; void *out[MEAO_MAX_BATCH]; meao_params prm[MEAO_MAX_BATCH]; meao_extent ext[MEAO_MAX_BATCH]; };
    FrameSet share(int32_t m, int32_t G, Storage *s) const
    {
        FrameSet mine = *this;
        int32_t k = 0;
        for (int32_t f = m; f < n; f += G, ++k) {
            s->depth[k] = depth[f];
            if (out) s->out[k] = out[f];
            if (params) s->prm[k] = params[f];
            if (extents) s->ext[k] = extents[f];
        }
        mine.n = k; mine.depth = s->depth; mine.out = out ? s->out : nullptr; mine.params = params ? s->prm : nullptr;
        mine.extents = extents ? s->ext : nullptr;
        return mine;
    }
};

// A composite's surfaces (gbuffer0 null = none; pitches in bytes, 0 = tightly packed).
struct CompositeTargets {
    int32_t mode, n;
    const void *const *ao; uint64_t ao_pitch;
    void *const *color; int32_t color_format; uint64_t color_pitch;
    void *const *gbuffer0; uint64_t gbuffer0_pitch;
    // meao_composite_batch_extents / meao_execute_batch_extents_shaded: frame f's own size and pitches (the three pitches above
    // are then unused); null = every frame has the context's size.  from_arrays: the shaded call made them from its extents[],
    // color_pitch[] and gbuffer0_pitch[], which is how its errors name them.
    const meao_target_extent *extents = nullptr;
    bool from_arrays = false;

    struct Storage { const void *ao[MEAO_MAX_BATCH]; void *color[MEAO_MAX_BATCH]; void *gbuffer0[MEAO_MAX_BATCH]; meao_target_extent ext[MEAO_MAX_BATCH]; };
    CompositeTargets share(int32_t m, int32_t G, Storage *s) const
    {
        CompositeTargets mine = *this;
        int32_t k = 0;
        for (int32_t f = m; f < n; f += G, ++k) {
            if (ao) s->ao[k] = ao[f];
            s->color[k] = color[f];
            if (gbuffer0) s->gbuffer0[k] = gbuffer0[f];
            if (extents) s->ext[k] = extents[f];
        }
        mine.n = k; mine.ao = ao ? s->ao : nullptr; mine.color = s->color; mine.gbuffer0 = gbuffer0 ? s->gbuffer0 : nullptr;
        mine.extents = extents ? s->ext : nullptr;
        return mine;
    }
};

// ---- meao_api.cpp
int use_device(meao_ctx *ctx);
bool exact_rcp_div_applicable(const meao_config &c, const Plan &plan);
// (Re)plans for cfg/two_ds_sets and replaces the arena, laid out for cap_w x cap_h (0, 0: for cfg's size, and the context then
// holds no reservation); on failure the context is untouched.
int reallocate(meao_ctx *ctx, const meao_config &cfg, bool two_ds_sets, int32_t cap_w, int32_t cap_h);
// What config_valid says of a frame size.
bool size_valid(int32_t width, int32_t height);

// ---- meao_execute.cpp
// Every params[f] valid (as meao_set_params checks it); else the status, with the frame named in the context's error.
int validate_frame_params(meao_ctx *ctx, int32_t n, const meao_params *params, const char *what);
// A row pitch (bytes, 0 = tightly packed) -> the row stride in texels; `what` names the argument in the error.
int pitch_texels(meao_ctx *ctx, uint64_t pitch, uint64_t elem, const char *what, int32_t *out);
// The same for frames of width x height instead of the context's size (meao_prefetch_batch_sized).
int pitch_texels_of(meao_ctx *ctx, int32_t width, int32_t height, uint64_t pitch, uint64_t elem, const char *what, int32_t *out);
// Every check of an execute call, before anything is enqueued; the row strides in texels on success.
int validate_execute_batch(meao_ctx *ctx, const FrameSet &fs, int32_t *depth_rows, int32_t *out_rows);
// Every check of meao_execute_batch_extents (fs.extents set, DEVICE surfaces), before anything is enqueued; on success each
// frame's row strides in texels.  *uniform: every extent is the context's size and all frames share their pitches -- the call is
// meao_execute_batch_pitched with extents[0]'s.
int validate_execute_batch_extents(meao_ctx *ctx, const FrameSet &fs, int32_t *depth_rows, int32_t *out_rows, bool *uniform);
// For meao_pool.cpp too: meao_execute_batch* (fs.extents set: meao_execute_batch_extents); wait_for_host = false (pool members only) leaves the staged copies of a HOST
// call in flight on `stream` -- the caller synchronises the stream before it touches the host buffers.
int execute_batch_internal(meao_ctx *ctx, const FrameSet &fs, meao_stream stream, bool wait_for_host);
// For meao_pool.cpp too: meao_prefetch_batch* without the checks of params[] (the caller made them): fs.n, depth, depth_pitch, params.
// width x height: the announced frames' size (meao_prefetch_batch_sized), 0 x 0 = the context's.
int prefetch_batch_internal(meao_ctx *ctx, const FrameSet &fs, int32_t width = 0, int32_t height = 0);
// For meao_pool.cpp: what a member that is dealt no frame of a pool call does instead of that call.
// ready_too = false (a pool announcement passed it by): an announcement it still holds is withdrawn, as a newer one would
// replace it.  ready_too = true (a pool execute passed it by): a ready prefetched set goes as well -- the pool-level "call
// after next" any of them was made for is over.  Bookkeeping only; costs that member one downsample pass at most.
void drop_announcement(meao_ctx *ctx, bool ready_too);

// ---- meao_composite.cpp
// Runs a pending composite batch as plain composite launches (one per frame) on `stream`.
int flush_pending_composite(meao_ctx *ctx, hipStream_t stream);
// For meao_pool.cpp too: meao_composite_enqueue_format under the name `fn` (the errors carry it); validate_only = every
// check and nothing else (no device is touched, a waiting batch stays as it is).
int composite_enqueue_internal(meao_ctx *ctx, const char *fn, const CompositeTargets &t, bool validate_only);
// For meao_pool.cpp too: meao_execute_batch_shaded under the name `fn` (t.ao / ao_pitch / n are taken from fs.out); validate_only
// = every check of both halves and nothing else (no device is touched; AO, colour, an announcement and a waiting batch stay).
int execute_batch_shaded_internal(meao_ctx *ctx, const char *fn, const FrameSet &fs, const CompositeTargets &t, meao_stream stream,
                                  bool validate_only);
// For meao_pool.cpp too: meao_execute_batch_extents_shaded under the name `fn`: fs.extents and t.extents set (t.extents[f]'s width,
// height and ao_pitch are fs.extents[f]'s; t.ao / n are taken from fs.out); validate_only as above.
int execute_batch_extents_shaded_internal(meao_ctx *ctx, const char *fn, const FrameSet &fs, const CompositeTargets &t, meao_stream stream,
                                          bool validate_only);
// Frame f's meao_target_extent of a shaded mixed call, from its three per-frame arguments (pitch arrays null = tightly packed).
inline meao_target_extent target_extent_of(const meao_extent &e, const uint64_t *color_pitch, const uint64_t *gbuffer0_pitch, int32_t f)
{
    return meao_target_extent{e.width, e.height, e.ao_pitch, color_pitch ? color_pitch[f] : 0, gbuffer0_pitch ? gbuffer0_pitch[f] : 0};
}

}  // namespace meao
