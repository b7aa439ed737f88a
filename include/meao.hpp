// meao.hpp -- header-only C++ host side over the C ABI of libmeao_hip.so (include/meao.h).
//
// The reference's host side is a compiled C# component, MiniEngineAO.AmbientOcclusion
// (Assets/MiniEngineAO/AmbientOcclusion.cs, "AO.cs").  No C# toolchain exists in the build
// image, so the compiled-language host mirror is this C++ class (the C# P/Invoke source a
// maintainer would add is bindings/csharp/).  Same six public properties, same names and
// defaults (AO.cs:20-68); camera terms, depth input and AO output are explicit.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "meao.h"

namespace MiniEngineAO {

class Error : public std::runtime_error {
public:
    Error(int32_t status, const std::string &what) : std::runtime_error(what), status_(status) {}
    int32_t status() const { return status_; }

private:
    int32_t status_;
};

class AmbientOcclusion {
public:
    // ---- Exposed properties (AO.cs:20-68) ---------------------------------------------------
    float noiseFilterTolerance = 0.0f;   // Range(-8, 0)
    float blurTolerance = -4.6f;         // Range(-8, -1)
    float upsampleTolerance = -12.0f;    // Range(-12, -1)
    float thicknessModifier = 1.0f;      // Range(1, 10)
    float intensity = 1.0f;              // Range(0, 2)
    bool ambientOnly = true;             // composite-side flag (AO.cs:62-68)
    // the camera target's format for CompositeFormat / CompositeWithNextFrameFormat; the HDR one (ARGBHalf) by default
    meao_color_format colorFormat = MEAO_COLOR_RGBA16F;

    // ---- camera terms Unity supplied implicitly (AO.cs:563-573) -----------------------------
    float nearClipPlane = 0.3f;
    float farClipPlane = 1000.0f;
    float projection00 = 0.9742786f;     // camera.projectionMatrix[0,0]
    bool usesReversedZBuffer = true;
    bool singlePassStereoEnabled = false;   // AO.cs:392-401: pixelWidth is then the double-wide eye pair

    // hqLevels / sampleSet: variants the reference's shaders carry but its host never dispatches
    // (Render.main wide + Upsample.main_premin*, SAMPLE_EXHAUSTIVELY); 0 = the reference's wiring.
    AmbientOcclusion(int32_t pixelWidth, int32_t pixelHeight, int32_t device = 0,
                     meao_ao_format aoFormat = MEAO_AO_R8, int32_t maxBatch = 1, int32_t numLevels = 4,
                     meao_f16_rounding f16Rounding = MEAO_F16_RTZ_CLAMP,
                     meao_depth_format depthFormat = MEAO_DEPTH_F32, int32_t hqLevels = 0,   // MEAO_DEPTH_LINEAR_*: view-space z (meao.h)
                     meao_sample_set sampleSet = MEAO_SAMPLES_CHECKER)
    {
        meao_default_config(&cfg_);
        cfg_.device = device;
        cfg_.width = pixelWidth;
        cfg_.height = pixelHeight;
        cfg_.ao_format = aoFormat;
        cfg_.max_batch = maxBatch;
        cfg_.num_levels = numLevels;
        cfg_.f16_rounding = f16Rounding;
        cfg_.depth_format = depthFormat;
        cfg_.hq_levels = hqLevels;
        cfg_.sample_set = sampleSet;
        const int32_t rc = meao_create(&cfg_, &ctx_);
        if (rc != MEAO_OK) throw Error(rc, meao_last_error(nullptr));
    }
    AmbientOcclusion(const AmbientOcclusion &) = delete;
    AmbientOcclusion &operator=(const AmbientOcclusion &) = delete;
    ~AmbientOcclusion() { meao_destroy(ctx_); }   // OnDestroy (AO.cs:357-381); discards a composite still waiting (FlushComposite first)

    int32_t width() const { return cfg_.width; }
    int32_t height() const { return cfg_.height; }
    size_t aoTexelBytes() const { return cfg_.ao_format == MEAO_AO_R8 ? 1 : 2; }

    // Device-resident depth in -> AO texture out, asynchronous on `stream`
    // (replays what RebuildCommandBuffers records, AO.cs:496-531).
    void Render(const void *deviceDepth, void *deviceAo, meao_stream stream = nullptr)
    {
        sync();
        check(meao_execute(ctx_, deviceDepth, MEAO_MEM_DEVICE, deviceAo, MEAO_MEM_DEVICE, stream));
    }

    void RenderBatch(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                     meao_stream stream = nullptr)
    {
        sync();
        check(meao_execute_batch(ctx_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(),
                                 MEAO_MEM_DEVICE, deviceAo.data(), MEAO_MEM_DEVICE, stream));
    }

    // Host arrays in and out (synchronous).
    void RenderHost(const void *depth, void *ao)
    {
        sync();
        check(meao_execute(ctx_, depth, MEAO_MEM_HOST, ao, MEAO_MEM_HOST, nullptr));
    }

    void Resize(int32_t pixelWidth, int32_t pixelHeight)   // screen-size change (AO.cs:338-341)
    {
        check(meao_resize(ctx_, pixelWidth, pixelHeight));
        cfg_.width = pixelWidth;
        cfg_.height = pixelHeight;
    }
    // Dynamic resolution: reserve the maximum size once (it may allocate and synchronises the device once); Resize to any size
    // inside it then moves nothing -- no allocation, no synchronisation (meao_reserve).  (0, 0) drops the reservation.
    void Reserve(int32_t maxWidth, int32_t maxHeight) { check(meao_reserve(ctx_, maxWidth, maxHeight)); }
    void Capacity(int32_t *width, int32_t *height) { check(meao_get_capacity(ctx_, width, height)); }   // (0, 0) = no reservation
    uint64_t ReserveBytes(int32_t maxWidth, int32_t maxHeight)    // the device memory such a reservation costs
    {
        uint64_t bytes = 0;
        check(meao_reserve_bytes(&cfg_, maxWidth, maxHeight, &bytes));
        return bytes;
    }
    // The announcement for frames of width x height, a size inside the reservation: Resize(width, height) keeps it
    // (meao_prefetch_batch_sized).  depthPitch 0 = tightly packed.
    void PrefetchBatchSized(int32_t width, int32_t height, const std::vector<const void *> &nextDeviceDepth, uint64_t depthPitch = 0,
                            const std::vector<meao_params> &params = {})
    {
        if (!params.empty() && params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        sync();
        check(meao_prefetch_batch_sized(ctx_, width, height, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(), depthPitch,
                                        params.empty() ? nullptr : params.data()));
    }

    // Streams of frames: announce the device depth frames of the call after next; the next Render*
    // carries their downsample pass inside its last kernel (meao_prefetch_batch).
    void PrefetchBatch(const std::vector<const void *> &nextDeviceDepth)
    {
        sync();   // pending property changes first: meao_set_params would drop the announcement
        check(meao_prefetch_batch(ctx_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data()));
    }

    // Several cameras in one batch: frame f uses params[f] (meao_execute_batch_params); the instance's own parameters are neither
    // read nor changed.  PrefetchBatchParams announces the next batch with its frames' parameters (meao_prefetch_batch_params).
    void RenderBatchParams(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                           const std::vector<meao_params> &params, meao_stream stream = nullptr)
    {
        if (params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_execute_batch_params(ctx_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), MEAO_MEM_DEVICE,
                                        deviceAo.data(), MEAO_MEM_DEVICE, params.data(), stream));
    }
    void PrefetchBatchParams(const std::vector<const void *> &nextDeviceDepth, const std::vector<meao_params> &params)
    {
        if (params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_prefetch_batch_params(ctx_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(), params.data()));
    }

    // Row-pitched device surfaces (meao_execute_batch_pitched): pitches in bytes, 0 = tightly packed; params empty = the instance's
    // parameters, else one per frame.
    void RenderBatchPitched(const std::vector<const void *> &deviceDepth, uint64_t depthPitch, const std::vector<void *> &deviceAo,
                            uint64_t aoPitch, const std::vector<meao_params> &params = {}, meao_stream stream = nullptr)
    {
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_execute_batch_pitched(ctx_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), depthPitch, MEAO_MEM_DEVICE,
                                         deviceAo.data(), aoPitch, MEAO_MEM_DEVICE, params.empty() ? nullptr : params.data(), stream));
    }
    // A mixed-size batch of device surfaces (meao_execute_batch_extents): extents[f] = frame f's own width, height and row
    // pitches (bytes, 0 = packed for that width), every size inside the reservation, else inside this instance's size; params
    // empty = the instance's parameters, else one per frame.
    void RenderBatchExtents(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                            const std::vector<meao_extent> &extents, const std::vector<meao_params> &params = {}, meao_stream stream = nullptr)
    {
        if (extents.size() != deviceDepth.size() || deviceAo.size() != deviceDepth.size())
            throw std::invalid_argument("meao: one AO surface and one meao_extent per frame");
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        sync();
        check(meao_execute_batch_extents(ctx_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), deviceAo.data(), extents.data(),
                                         params.empty() ? nullptr : params.data(), stream));
    }
    void PrefetchBatchPitched(const std::vector<const void *> &nextDeviceDepth, uint64_t depthPitch,
                              const std::vector<meao_params> &params = {})
    {
        if (!params.empty() && params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        sync();
        check(meao_prefetch_batch_pitched(ctx_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(), depthPitch,
                                          params.empty() ? nullptr : params.data()));
    }

    void Synchronize(meao_stream stream = nullptr) { check(meao_synchronize(ctx_, stream)); }

    // PushCompositeCommands (AO.cs:822-839).  Composite(): now, on `stream`.  CompositeWithNextFrame(): the
    // composite of device frames this component produced rides inside the render kernel of the next
    // Render* call (meao_composite_enqueue); FlushComposite() runs whatever still waits.
    void Composite(meao_composite_mode mode, const void *deviceAo, void *deviceColorRgba16f, void *deviceGBuffer0 = nullptr,
                   meao_stream stream = nullptr)
    {
        check(meao_composite(ctx_, mode, deviceAo, deviceColorRgba16f, deviceGBuffer0, MEAO_MEM_DEVICE, stream));
    }
    void CompositeWithNextFrame(meao_composite_mode mode, const std::vector<const void *> &deviceAo,
                                const std::vector<void *> &deviceColorRgba16f, const std::vector<void *> &deviceGBuffer0 = {})
    {
        check(meao_composite_enqueue(ctx_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), deviceColorRgba16f.data(),
                                     deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data()));
    }
    // The same into row-pitched surfaces (meao_composite_pitched / meao_composite_enqueue_pitched): pitches in bytes, 0 = tightly packed.
    void CompositePitched(meao_composite_mode mode, const void *deviceAo, uint64_t aoPitch, void *deviceColorRgba16f, uint64_t colorPitch,
                          void *deviceGBuffer0 = nullptr, uint64_t gbuffer0Pitch = 0, meao_stream stream = nullptr)
    {
        check(meao_composite_pitched(ctx_, mode, deviceAo, aoPitch, deviceColorRgba16f, colorPitch, deviceGBuffer0, gbuffer0Pitch,
                                     MEAO_MEM_DEVICE, stream));
    }
    void CompositeWithNextFramePitched(meao_composite_mode mode, const std::vector<const void *> &deviceAo, uint64_t aoPitch,
                                       const std::vector<void *> &deviceColorRgba16f, uint64_t colorPitch,
                                       const std::vector<void *> &deviceGBuffer0 = {}, uint64_t gbuffer0Pitch = 0)
    {
        check(meao_composite_enqueue_pitched(ctx_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), aoPitch,
                                             deviceColorRgba16f.data(), colorPitch, deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(),
                                             gbuffer0Pitch));
    }
    // The same into colour targets in `colorFormat` (meao_composite_format / meao_composite_enqueue_format): RGBA16F, RGBA32F, RGBA8,
    // R11G11B10F or -- the LDR target of a linear-colour-space project -- RGBA8_SRGB.  A batch in another format than RGBA16F does not ride in the render kernel: the next Render* call runs it first.
    void CompositeFormat(meao_composite_mode mode, const void *deviceAo, uint64_t aoPitch, void *deviceColor, uint64_t colorPitch,
                         void *deviceGBuffer0 = nullptr, uint64_t gbuffer0Pitch = 0, meao_stream stream = nullptr)
    {
        check(meao_composite_format(ctx_, mode, deviceAo, aoPitch, deviceColor, colorFormat, colorPitch, deviceGBuffer0, gbuffer0Pitch,
                                    MEAO_MEM_DEVICE, stream));
    }
    void CompositeWithNextFrameFormat(meao_composite_mode mode, const std::vector<const void *> &deviceAo, uint64_t aoPitch,
                                      const std::vector<void *> &deviceColor, uint64_t colorPitch,
                                      const std::vector<void *> &deviceGBuffer0 = {}, uint64_t gbuffer0Pitch = 0)
    {
        check(meao_composite_enqueue_format(ctx_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), aoPitch, deviceColor.data(),
                                            colorFormat, colorPitch, deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch));
    }
    // The whole batch in ONE launch on `stream`, now (meao_composite_batch): nothing waits afterwards, a waiting batch is left alone.
    void CompositeBatch(meao_composite_mode mode, const std::vector<const void *> &deviceAo, uint64_t aoPitch,
                        const std::vector<void *> &deviceColor, uint64_t colorPitch, const std::vector<void *> &deviceGBuffer0 = {},
                        uint64_t gbuffer0Pitch = 0, meao_stream stream = nullptr)
    {
        check(meao_composite_batch(ctx_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), aoPitch, deviceColor.data(),
                                   colorFormat, colorPitch, deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch, stream));
    }
    // The batch in ONE launch with one size and one set of pitches per frame (meao_composite_batch_extents): extents[f] = frame
    // f's width, height and the row pitches of its three surfaces (bytes, 0 = packed for that width); any size, no capacity rule.
    void CompositeBatchExtents(meao_composite_mode mode, const std::vector<const void *> &deviceAo, const std::vector<void *> &deviceColor,
                               const std::vector<meao_target_extent> &extents, const std::vector<void *> &deviceGBuffer0 = {},
                               meao_stream stream = nullptr)
    {
        if (deviceColor.size() != deviceAo.size() || extents.size() != deviceAo.size() ||
            (!deviceGBuffer0.empty() && deviceGBuffer0.size() != deviceAo.size()))
            throw std::invalid_argument("meao: one colour surface and one meao_target_extent per frame");
        check(meao_composite_batch_extents(ctx_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), deviceColor.data(), colorFormat,
                                           deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), extents.data(), stream));
    }
    // AO and shaded frames from one mixed-size call (meao_execute_batch_extents_shaded): RenderBatchExtents, then that composite
    // of deviceAo[f] into deviceColor[f] on the same stream.  targets[f] = frame f's width, height and the pitches of its AO,
    // colour and GBuffer0 surfaces; depthPitch empty = every depth frame packed, else one pitch per frame.
    void RenderDeviceBatchExtentsShaded(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                                        const std::vector<meao_target_extent> &targets, meao_composite_mode mode,
                                        const std::vector<void *> &deviceColor, const std::vector<void *> &deviceGBuffer0 = {},
                                        const std::vector<uint64_t> &depthPitch = {}, const std::vector<meao_params> &params = {},
                                        meao_stream stream = nullptr)
    {
        const size_t n = deviceDepth.size();
        if (deviceAo.size() != n || deviceColor.size() != n || targets.size() != n || (!deviceGBuffer0.empty() && deviceGBuffer0.size() != n))
            throw std::invalid_argument("meao: one AO surface, one colour surface and one meao_target_extent per frame");
        if (!depthPitch.empty() && depthPitch.size() != n) throw std::invalid_argument("meao: one depth pitch per frame");
        if (!params.empty() && params.size() != n) throw std::invalid_argument("meao: one meao_params per frame");
        std::vector<meao_extent> extents(n);
        std::vector<uint64_t> colorPitch(n), gbuffer0Pitch(n);
        for (size_t f = 0; f < n; ++f) {
            extents[f] = meao_extent{targets[f].width, targets[f].height, depthPitch.empty() ? 0 : depthPitch[f], targets[f].ao_pitch};
            colorPitch[f] = targets[f].color_pitch; gbuffer0Pitch[f] = targets[f].gbuffer0_pitch;
        }
        sync();
        check(meao_execute_batch_extents_shaded(ctx_, static_cast<int32_t>(n), deviceDepth.data(), deviceAo.data(), extents.data(),
                                                params.empty() ? nullptr : params.data(), mode, deviceColor.data(), colorFormat,
                                                colorPitch.data(), deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(),
                                                gbuffer0Pitch.data(), stream));
    }
    // AO and shaded frames from one call (meao_execute_batch_shaded): RenderDeviceBatchPitched, then the batched composite of
    // deviceAo[f] into deviceColor[f] on the same stream.  params empty = the context's parameters.
    void RenderDeviceBatchShaded(const std::vector<const void *> &deviceDepth, uint64_t depthPitch, const std::vector<void *> &deviceAo,
                                 uint64_t aoPitch, meao_composite_mode mode, const std::vector<void *> &deviceColor, uint64_t colorPitch,
                                 const std::vector<void *> &deviceGBuffer0 = {}, uint64_t gbuffer0Pitch = 0,
                                 const std::vector<meao_params> &params = {}, meao_stream stream = nullptr)
    {
        if (deviceAo.size() != deviceDepth.size() || deviceColor.size() != deviceDepth.size())
            throw std::invalid_argument("meao: one AO and one colour surface per frame");
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_execute_batch_shaded(ctx_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), depthPitch, deviceAo.data(),
                                        aoPitch, params.empty() ? nullptr : params.data(), mode, deviceColor.data(), colorFormat, colorPitch,
                                        deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch, stream));
    }
    void FlushComposite(meao_stream stream = nullptr) { check(meao_composite_flush(ctx_, stream)); }
    bool CompositePending()            // a batch given to CompositeWithNextFrame that no Render* / flush / resize has run yet
    {
        int32_t frames = 0;
        check(meao_composite_pending(ctx_, &frames));
        return frames > 0;
    }

    // roctx ranges per pass for rocprofv3 --marker-trace
    void SetTracing(bool enable) { check(meao_set_tracing(ctx_, enable ? 1 : 0)); }

    // The _debug 1..17 views (AO.cs:787-820) and OcclusionHQ1..4 (18..21), copied to the host.
    std::vector<uint8_t> DebugBuffer(int32_t debugId, meao_desc *desc = nullptr, int32_t frame = 0)
    {
        meao_desc d{};
        check(meao_get_intermediate(ctx_, frame, debugId, nullptr, 0, MEAO_MEM_HOST, &d));
        std::vector<uint8_t> data(d.bytes);
        check(meao_get_intermediate(ctx_, frame, debugId, data.data(), d.bytes, MEAO_MEM_HOST, &d));
        if (desc) *desc = d;
        return data;
    }

    // Bit f = frame f of the last Render* held NaN / inf / out-of-range depth texels and ran the IEEE-division bodies.
    uint64_t HostileFrames()
    {
        uint64_t mask = 0;
        check(meao_hostile_frames(ctx_, &mask));
        return mask;
    }

    meao_ctx *native() { return ctx_; }

private:
    void sync()   // CheckPropertiesChanged (AO.cs:104-113): push only what changed
    {
        meao_params p;
        meao_default_params(&p);
        p.noise_filter_tolerance = noiseFilterTolerance;
        p.blur_tolerance = blurTolerance;
        p.upsample_tolerance = upsampleTolerance;
        p.thickness_modifier = thicknessModifier;
        p.intensity = intensity;
        p.near_clip = nearClipPlane;
        p.far_clip = farClipPlane;
        p.proj00 = projection00;
        p.reversed_z = usesReversedZBuffer ? 1 : 0;
        p.single_pass_stereo = singlePassStereoEnabled ? 1 : 0;
        if (!applied_valid_ || !same(p, applied_)) {
            check(meao_set_params(ctx_, &p));
            applied_ = p;
            applied_valid_ = true;
        }
    }
    static bool same(const meao_params &a, const meao_params &b)
    {
        return a.noise_filter_tolerance == b.noise_filter_tolerance && a.blur_tolerance == b.blur_tolerance &&
               a.upsample_tolerance == b.upsample_tolerance && a.thickness_modifier == b.thickness_modifier &&
               a.intensity == b.intensity && a.near_clip == b.near_clip && a.far_clip == b.far_clip &&
               a.proj00 == b.proj00 && a.reversed_z == b.reversed_z && a.single_pass_stereo == b.single_pass_stereo;
    }
    void check(int32_t rc)
    {
        if (rc == MEAO_OK) return;
        std::string msg = meao_last_error(ctx_);
        if (msg.empty()) msg = meao_status_string(rc);
        throw Error(rc, msg);
    }

    meao_ctx *ctx_ = nullptr;
    meao_config cfg_{};
    meao_params applied_{};
    bool applied_valid_ = false;
};

// One context per device behind meao_pool_*: frame f of a batch runs on member f mod G (the in-process multi-GPU host;
// SURVEY 8e).  `devices` may repeat an ordinal (several members on one GPU: a throughput mode of its own).
class AmbientOcclusionPool {
public:
    AmbientOcclusionPool(int32_t pixelWidth, int32_t pixelHeight, const std::vector<int32_t> &devices, int32_t maxBatchPerMember = 1,
                         meao_ao_format aoFormat = MEAO_AO_R8, bool pipelined = false)
    {
        meao_config cfg;
        meao_default_config(&cfg);
        cfg.width = pixelWidth;
        cfg.height = pixelHeight;
        cfg.ao_format = aoFormat;
        cfg.max_batch = maxBatchPerMember;
        cfg.pipelined = pipelined ? 1 : 0;
        const int32_t rc = meao_pool_create(&cfg, devices.data(), static_cast<int32_t>(devices.size()), &pool_);
        if (rc != MEAO_OK) throw Error(rc, meao_pool_last_error(nullptr));
    }
    AmbientOcclusionPool(const AmbientOcclusionPool &) = delete;
    AmbientOcclusionPool &operator=(const AmbientOcclusionPool &) = delete;
    ~AmbientOcclusionPool() { meao_pool_destroy(pool_); }

    int32_t Size() const { return meao_pool_size(pool_); }
    int32_t DeviceOfFrame(int32_t frame) const { return meao_pool_device_of_frame(pool_, frame); }
    void SetParams(const meao_params &p) { check(meao_pool_set_params(pool_, &p)); }
    // Frame f resident on DeviceOfFrame(f); asynchronous (Synchronize()).
    void RenderDeviceBatch(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo)
    {
        check(meao_pool_execute_batch(pool_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), MEAO_MEM_DEVICE,
                                      deviceAo.data(), MEAO_MEM_DEVICE));
    }
    // Dynamic resolution (meao_pool_reserve / meao_pool_resize / meao_pool_prefetch_batch_sized): Resize takes sizes every
    // member's reservation covers, and then neither allocates nor synchronises.
    void Reserve(int32_t maxWidth, int32_t maxHeight) { check(meao_pool_reserve(pool_, maxWidth, maxHeight)); }
    void Resize(int32_t width, int32_t height) { check(meao_pool_resize(pool_, width, height)); }
    void PrefetchBatchSized(int32_t width, int32_t height, const std::vector<const void *> &nextDeviceDepth, uint64_t depthPitch = 0,
                            const std::vector<meao_params> &params = {})
    {
        if (!params.empty() && params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_prefetch_batch_sized(pool_, width, height, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(),
                                             depthPitch, params.empty() ? nullptr : params.data()));
    }
    void PrefetchBatch(const std::vector<const void *> &nextDeviceDepth)
    {
        check(meao_pool_prefetch_batch(pool_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data()));
    }
    // per-frame parameters: params[f] goes with frame f to member f mod G
    void RenderDeviceBatchParams(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                                 const std::vector<meao_params> &params)
    {
        if (params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_execute_batch_params(pool_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), MEAO_MEM_DEVICE,
                                             deviceAo.data(), MEAO_MEM_DEVICE, params.data()));
    }
    void PrefetchBatchParams(const std::vector<const void *> &nextDeviceDepth, const std::vector<meao_params> &params)
    {
        if (params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_prefetch_batch_params(pool_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(),
                                              params.data()));
    }
    // the composite of device frames into row-pitched surfaces, carried by the members' next calls (meao_pool_composite_enqueue_pitched)
    void CompositeWithNextFramePitched(meao_composite_mode mode, const std::vector<const void *> &deviceAo, uint64_t aoPitch,
                                       const std::vector<void *> &deviceColorRgba16f, uint64_t colorPitch,
                                       const std::vector<void *> &deviceGBuffer0 = {}, uint64_t gbuffer0Pitch = 0)
    {
        check(meao_pool_composite_enqueue_pitched(pool_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), aoPitch,
                                                  deviceColorRgba16f.data(), colorPitch,
                                                  deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch));
    }
    // the same into colour targets of another format (meao_pool_composite_enqueue_format)
    void CompositeWithNextFrameFormat(meao_composite_mode mode, const std::vector<const void *> &deviceAo, uint64_t aoPitch,
                                      const std::vector<void *> &deviceColor, meao_color_format colorFormat, uint64_t colorPitch,
                                      const std::vector<void *> &deviceGBuffer0 = {}, uint64_t gbuffer0Pitch = 0)
    {
        check(meao_pool_composite_enqueue_format(pool_, mode, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), aoPitch,
                                                 deviceColor.data(), colorFormat, colorPitch,
                                                 deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch));
    }
    // AO and shaded frames from one pool call (meao_pool_execute_batch_shaded): one batched composite launch per member
    void RenderDeviceBatchShaded(const std::vector<const void *> &deviceDepth, uint64_t depthPitch, const std::vector<void *> &deviceAo,
                                 uint64_t aoPitch, meao_composite_mode mode, const std::vector<void *> &deviceColor,
                                 meao_color_format colorFormat, uint64_t colorPitch, const std::vector<void *> &deviceGBuffer0 = {},
                                 uint64_t gbuffer0Pitch = 0, const std::vector<meao_params> &params = {})
    {
        if (deviceAo.size() != deviceDepth.size() || deviceColor.size() != deviceDepth.size())
            throw std::invalid_argument("meao: one AO and one colour surface per frame");
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_execute_batch_shaded(pool_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), depthPitch, deviceAo.data(),
                                             aoPitch, params.empty() ? nullptr : params.data(), mode, deviceColor.data(), colorFormat,
                                             colorPitch, deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(), gbuffer0Pitch));
    }
    // AO and shaded frames from one mixed-size pool call (meao_pool_execute_batch_extents_shaded): targets[f] and depthPitch[f] go
    // with frame f to member f mod G; arguments as AmbientOcclusion::RenderDeviceBatchExtentsShaded
    void RenderDeviceBatchExtentsShaded(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                                        const std::vector<meao_target_extent> &targets, meao_composite_mode mode,
                                        const std::vector<void *> &deviceColor, meao_color_format colorFormat,
                                        const std::vector<void *> &deviceGBuffer0 = {}, const std::vector<uint64_t> &depthPitch = {},
                                        const std::vector<meao_params> &params = {})
    {
        const size_t n = deviceDepth.size();
        if (deviceAo.size() != n || deviceColor.size() != n || targets.size() != n || (!deviceGBuffer0.empty() && deviceGBuffer0.size() != n))
            throw std::invalid_argument("meao: one AO surface, one colour surface and one meao_target_extent per frame");
        if (!depthPitch.empty() && depthPitch.size() != n) throw std::invalid_argument("meao: one depth pitch per frame");
        if (!params.empty() && params.size() != n) throw std::invalid_argument("meao: one meao_params per frame");
        std::vector<meao_extent> extents(n);
        std::vector<uint64_t> colorPitch(n), gbuffer0Pitch(n);
        for (size_t f = 0; f < n; ++f) {
            extents[f] = meao_extent{targets[f].width, targets[f].height, depthPitch.empty() ? 0 : depthPitch[f], targets[f].ao_pitch};
            colorPitch[f] = targets[f].color_pitch; gbuffer0Pitch[f] = targets[f].gbuffer0_pitch;
        }
        check(meao_pool_execute_batch_extents_shaded(pool_, static_cast<int32_t>(n), deviceDepth.data(), deviceAo.data(), extents.data(),
                                                     params.empty() ? nullptr : params.data(), mode, deviceColor.data(), colorFormat,
                                                     colorPitch.data(), deviceGBuffer0.empty() ? nullptr : deviceGBuffer0.data(),
                                                     gbuffer0Pitch.data()));
    }
    // row-pitched device surfaces (meao_pool_execute_batch_pitched); params empty = the members' own parameters
    void RenderDeviceBatchPitched(const std::vector<const void *> &deviceDepth, uint64_t depthPitch, const std::vector<void *> &deviceAo,
                                  uint64_t aoPitch, const std::vector<meao_params> &params = {})
    {
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_execute_batch_pitched(pool_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), depthPitch,
                                              MEAO_MEM_DEVICE, deviceAo.data(), aoPitch, MEAO_MEM_DEVICE,
                                              params.empty() ? nullptr : params.data()));
    }
    // a mixed-size batch (meao_pool_execute_batch_extents): extents[f] goes with frame f to member f mod G
    void RenderDeviceBatchExtents(const std::vector<const void *> &deviceDepth, const std::vector<void *> &deviceAo,
                                  const std::vector<meao_extent> &extents, const std::vector<meao_params> &params = {})
    {
        if (extents.size() != deviceDepth.size() || deviceAo.size() != deviceDepth.size())
            throw std::invalid_argument("meao: one AO surface and one meao_extent per frame");
        if (!params.empty() && params.size() != deviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_execute_batch_extents(pool_, static_cast<int32_t>(deviceDepth.size()), deviceDepth.data(), deviceAo.data(),
                                              extents.data(), params.empty() ? nullptr : params.data()));
    }
    void PrefetchBatchPitched(const std::vector<const void *> &nextDeviceDepth, uint64_t depthPitch,
                              const std::vector<meao_params> &params = {})
    {
        if (!params.empty() && params.size() != nextDeviceDepth.size()) throw std::invalid_argument("meao: one meao_params per frame");
        check(meao_pool_prefetch_batch_pitched(pool_, static_cast<int32_t>(nextDeviceDepth.size()), nextDeviceDepth.data(), depthPitch,
                                               params.empty() ? nullptr : params.data()));
    }
    void GatherToDevice(const std::vector<const void *> &deviceAo, const std::vector<void *> &dst, int32_t dstDevice)
    {
        check(meao_pool_gather_to_device(pool_, static_cast<int32_t>(deviceAo.size()), deviceAo.data(), dst.data(), dstDevice));
    }
    meao_pool_path GatherPath(int32_t member, int32_t dstDevice) const
    {
        return static_cast<meao_pool_path>(meao_pool_gather_path(pool_, member, dstDevice));
    }
    void Synchronize() { check(meao_pool_synchronize(pool_)); }
    // MEAO_POOL_SPIN_US / MEAO_POOL_BIND_NUMA (the workers bind themselves to their device's NUMA node; before the first device batch)
    void Configure(meao_pool_option key, int32_t value) { check(meao_pool_configure(pool_, key, value)); }
    int32_t NumaNodeOfMember(int32_t member) const
    {
        int32_t node = -1;
        (void)meao_pool_member_placement(pool_, member, &node, nullptr);
        return node;
    }
    meao_pool *native() { return pool_; }

private:
    void check(int32_t rc)
    {
        if (rc != MEAO_OK) throw Error(rc, meao_pool_last_error(pool_));
    }
    meao_pool *pool_ = nullptr;
};

}  // namespace MiniEngineAO
