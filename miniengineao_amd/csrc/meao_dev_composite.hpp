// meao_dev_composite.hpp -- Blit.shader passes 1-3 on a texel pair (composite kernel and the composite carried by the render kernel).
#pragma once

#include "meao_dev.hpp"

namespace meao {
namespace {

// ------------------------------------------------------------------------------------------
// Composite (Blit.shader:66-134): pure streaming, 17 bytes per texel (RGBA16F read + write, AO).
// One lane = 4 texels = two 16-byte colour loads/stores + one 4-byte (R8) AO load.

__device__ __forceinline__ uint16_t f32_to_f16_rtne_bits(float x) { return f32_to_f16_bits<true>(x); }

// One texel: t = its four f16 channels, g = its GBuffer0 texel (touched in AMBIENT_ONLY mode only).
__device__ __forceinline__ void composite_texel(uint16_t *t, float ao, int32_t mode, uint8_t *g)
{
    if (mode == MEAO_COMPOSITE_DEBUG) {                          // pass 3: frag returns ao in every channel
        t[0] = t[1] = t[2] = t[3] = f32_to_f16_rtne_bits(ao);
    } else if (mode == MEAO_COMPOSITE_MULTIPLY) {                // pass 2: dst * src.a
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = f32_to_f16_rtne_bits(f16_bits_to_f32(t[k]) * ao);
    } else {                                                     // pass 1: dst * (1 - src), src = 1 - ao
        const float occ = 1.0f - ao;                             // Blit.shader:84
        const float keep = 1.0f - occ;                           // OneMinusSrcColor / OneMinusSrcAlpha
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = f32_to_f16_rtne_bits(f16_bits_to_f32(t[k]) * keep);
        g[3] = static_cast<uint8_t>(f32_to_unorm8(unorm8_to_f32(g[3]) * keep));      // GBuffer0.a = occlusion
    }
}

__device__ __forceinline__ void unpack_pair(const uint4v raw, uint16_t *c)
{
    c[0] = raw.x & 0xffffu; c[1] = raw.x >> 16; c[2] = raw.y & 0xffffu; c[3] = raw.y >> 16;
    c[4] = raw.z & 0xffffu; c[5] = raw.z >> 16; c[6] = raw.w & 0xffffu; c[7] = raw.w >> 16;
}

__device__ __forceinline__ uint4v pack_pair(const uint16_t *c)
{
    uint4v outv;
    outv.x = c[0] | (static_cast<uint32_t>(c[1]) << 16); outv.y = c[2] | (static_cast<uint32_t>(c[3]) << 16);
    outv.z = c[4] | (static_cast<uint32_t>(c[5]) << 16); outv.w = c[6] | (static_cast<uint32_t>(c[7]) << 16);
    return outv;
}

// Texel pair q (texels 2q, 2q+1) of one frame: one 16-byte colour load / store per lane.
template <int AOFMT>
__device__ __forceinline__ void composite_pair(const void *ao_base, void *color_base, void *gbuffer0_base, int64_t pixels,
                                               int32_t mode, int64_t q)
{
    typedef AoTexel<AOFMT> AO;
    typedef typename AO::type ao_t;
    const int64_t p0 = q * 2;
    const bool full = p0 + 1 < pixels;
    const ao_t *ap = static_cast<const ao_t *>(ao_base) + p0;
    float aov[2] = {1.0f, 1.0f};
    if (full) {
        const typename AO::type2 a2 = *reinterpret_cast<const typename AO::type2 *>(ap);
        aov[0] = AO::decode(a2.x); aov[1] = AO::decode(a2.y);
    } else {
        aov[0] = AO::decode(ap[0]);
    }
    uint16_t c[8] = {};
    uint16_t *cp = static_cast<uint16_t *>(color_base) + p0 * 4;
    if (full) {
        unpack_pair(*reinterpret_cast<const uint4v *>(cp), c);
    } else {
        for (int k = 0; k < 4; ++k) c[k] = cp[k];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (p0 + e >= pixels) break;
        composite_texel(c + 4 * e, aov[e], mode, static_cast<uint8_t *>(gbuffer0_base) + (p0 + e) * 4);
    }
    if (full) {
        *reinterpret_cast<uint4v *>(cp) = pack_pair(c);
    } else {
        for (int k = 0; k < 4; ++k) cp[k] = c[k];
    }
}

// The 2-D form: pair px (texels 2px, 2px + 1) of row `row`; a row has ceil(w / 2) pairs, the last one of an odd row is a half
// pair (pairs never run across a row end).  Byte offsets are 32-bit from the frame base (the limits of meao_composite_pitched).
// A full pair of a vector-eligible surface moves as in the packed form; anything else texel by texel, with the same results.
template <int AOFMT>
__device__ __forceinline__ void composite_pair(const void *ao_base, void *color_base, void *gbuffer0_base, const CompositePitches &p,
                                               int32_t mode, uint32_t row, uint32_t px)
{
    typedef AoTexel<AOFMT> AO;
    typedef typename AO::type ao_t;
    const uint32_t x0 = px * 2u;
    const ao_t *ap = at_byte_offset(static_cast<const ao_t *>(ao_base), (__umul24(row, p.ao) + x0) * static_cast<uint32_t>(sizeof(ao_t)));
    uint16_t *cp = at_byte_offset(static_cast<uint16_t *>(color_base), (__umul24(row, p.color) + x0) * 8u);
    uint8_t *gp = at_byte_offset(static_cast<uint8_t *>(gbuffer0_base), (__umul24(row, p.gbuffer0) + x0) * 4u);
    uint16_t c[8];
    if (p.vec && x0 + 1u < static_cast<uint32_t>(p.w)) {
        const typename AO::type2 a2 = *reinterpret_cast<const typename AO::type2 *>(ap);
        unpack_pair(*reinterpret_cast<const uint4v *>(cp), c);
        composite_texel(c, AO::decode(a2.x), mode, gp);
        composite_texel(c + 4, AO::decode(a2.y), mode, gp + 4);
        *reinterpret_cast<uint4v *>(cp) = pack_pair(c);
        return;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (x0 + e >= static_cast<uint32_t>(p.w)) break;
        uint16_t *t = cp + 4 * e;
        for (int k = 0; k < 4; ++k) c[k] = t[k];
        composite_texel(c, AO::decode(ap[e]), mode, gp + 4 * e);
        for (int k = 0; k < 4; ++k) t[k] = c[k];
    }
}

// All pairs of one row, dealt to `lanes` lanes (lane = this one's index among them).
template <int AOFMT>
__device__ __forceinline__ void composite_row(const void *ao_base, void *color_base, void *gbuffer0_base, const CompositePitches &p,
                                              int32_t mode, uint32_t row, uint32_t lane, uint32_t lanes)
{
    const uint32_t row_pairs = (static_cast<uint32_t>(p.w) + 1u) / 2u;
    for (uint32_t px = lane; px < row_pairs; px += lanes) composite_pair<AOFMT>(ao_base, color_base, gbuffer0_base, p, mode, row, px);
}

// ------------------------------------------------------------------------------------------
// The other colour formats (meao_composite_format): RGBA32F, RGBA8, R11G11B10F and RGBA8_SRGB targets, in composite_kernel behind
// one kernel-uniform branch.  One lane = 16 bytes of colour = one RGBA32F texel or four texels of a 4-byte format, and their AO in
// one load; rows are dealt as in the pitched RGBA16F form, a tightly packed frame is one long row dealt to the whole grid.

// Unsigned small floats (5-bit exponent of bias 15, M mantissa bits: 6 for R and G, 5 for B).  Every code is the f16 value of
// the same exponent and left-aligned mantissa, so the decode is the f16 one, exact.
template <int M>
__device__ __forceinline__ float ufloat_to_f32(uint32_t code) { return f16_bits_to_f32(static_cast<uint16_t>(code << (10 - M))); }

// f32 -> small float: NaN -> all ones, anything with the sign bit -> 0, round to nearest even with gradual underflow, past the
// largest finite code -> +inf (the output-merger rule of f32_to_f16_bits<true>, for a format without a sign).
template <int M>
__device__ __forceinline__ uint32_t f32_to_ufloat(float x)
{
    asm volatile("" : "+v"(x));              // the value itself, in a VGPR: no folding of the product that made it into what follows
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    constexpr uint32_t kInf = 31u << M;
    if ((u & 0x7fffffffu) > 0x7f800000u) return kInf | ((1u << M) - 1u);
    if (u >> 31) return 0u;
    if (u >= (113u << 23)) {                 // a normal number of the target (or +inf): rebias, round the 23 - M low bits away
        constexpr uint32_t kShift = 23 - M;
        const uint32_t v = u - (112u << 23);
        const uint32_t r = (v + ((1u << (kShift - 1)) - 1u) + ((v >> kShift) & 1u)) >> kShift;
        return min(r, kInf);
    }
    // below 2^-14: the f32 sum with 2^(9 - M) has the target's subnormal step as its unit in the last place, so the addition
    // rounds (to nearest even) and its low bits are the code -- 2^M, the smallest normal, where the value rounds up to 2^-14
    constexpr float kMagic = static_cast<float>(1u << (9 - M));
    return __builtin_bit_cast(uint32_t, x + kMagic) - __builtin_bit_cast(uint32_t, kMagic);
}

__device__ __forceinline__ uint32_t f32_to_r11g11b10f(float r, float g, float b)
{
    return f32_to_ufloat<6>(r) | (f32_to_ufloat<6>(g) << 11) | (f32_to_ufloat<5>(b) << 22);
}

// What a texel is multiplied by: MULTIPLY ao (pass 2), AMBIENT_ONLY 1 - (1 - ao) (pass 1); DEBUG does not multiply.
__device__ __forceinline__ float composite_factor(float ao, int32_t mode)
{
    if (mode == MEAO_COMPOSITE_MULTIPLY) return ao;
    const float occ = 1.0f - ao;             // Blit.shader:84
    return 1.0f - occ;                       // OneMinusSrcColor / OneMinusSrcAlpha
}

__device__ __forceinline__ uint32_t unorm8_times(uint32_t code, float f) { return f32_to_unorm8(unorm8_to_f32(code) * f); }

// One texel of each format, in registers.  RGBA8: r, g, b in the low three bytes, alpha in the top one.
__device__ __forceinline__ uint32_t composite_rgba8(uint32_t t, float ao, int32_t mode)
{
    if (mode == MEAO_COMPOSITE_DEBUG) return f32_to_unorm8(ao) * 0x01010101u;
    const float f = composite_factor(ao, mode);
    const uint32_t a = mode == MEAO_COMPOSITE_MULTIPLY ? unorm8_times(t >> 24, f) : t >> 24;
    return unorm8_times(t & 255u, f) | (unorm8_times((t >> 8) & 255u, f) << 8) | (unorm8_times((t >> 16) & 255u, f) << 16) | (a << 24);
}

// RGBA8_SRGB: r, g, b sRGB-encoded and blended in linear light, alpha as in RGBA8.  The two f32 tables of the format's definition
// (meao.h; meao_srgb_tables.inc) sit in the workgroup's dynamic LDS, the only LDS of the kernels that use them: 256 words of D,
// then T[1..255].  srgb_stage_tables copies them there; a barrier follows before the first lookup.
constexpr uint32_t kSrgbWords = 256u + 255u, kSrgbLdsBytes = 2048u;

__device__ __forceinline__ float *srgb_lds()
{
    extern __shared__ float meao_srgb_lds[];
    return meao_srgb_lds;
}

__device__ __forceinline__ void srgb_stage_tables(const uint32_t *words)
{
    float *lds = srgb_lds();
    for (uint32_t i = threadIdx.x; i < kSrgbWords; i += blockDim.x) lds[i] = __builtin_bit_cast(float, words[i]);
}

__device__ __forceinline__ float srgb_decode(uint32_t code) { return srgb_lds()[code]; }

// enc(x) = the number of k in 1..255 with x >= T[k].  The fast form: e = floor(255 s(x) + 1/4), s the inverse transfer function
// through v_log_f32 / v_exp_f32 -- with an estimate less than a quarter of a code from the real 255 s(x), e is enc(x) or one below
// it (enc is floor(255 s + 1/2) up to the f32 rounding of the thresholds), and ONE comparison against T[e + 1] decides.  NaN
// takes the power arm, leaves fmaxf as 0 and fails the comparison: 0.  meao_selftest(9) checks every f32 against a search over T.
__device__ __forceinline__ uint32_t srgb_encode(float x)
{
    const float lo = x * 3294.6f;                                                                    // 255 x 12.92 x
    const float hi = 269.025f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(x) * (1.0f / 2.4f)) - 14.025f;    // 255 (1.055 x^(1/2.4) - 0.055)
    const float y = (x <= 0.0031308f ? lo : hi) + 0.25f;
    const uint32_t e = static_cast<uint32_t>(__builtin_fminf(__builtin_fmaxf(y, 0.0f), 254.0f));
    return e + (x >= srgb_lds()[256u + e] ? 1u : 0u);                                               // [256 + e] = T[e + 1]
}

__device__ __forceinline__ uint32_t composite_rgba8_srgb(uint32_t t, float ao, int32_t mode)
{
    if (mode == MEAO_COMPOSITE_DEBUG) return srgb_encode(ao) * 0x00010101u | (f32_to_unorm8(ao) << 24);
    const float f = composite_factor(ao, mode);
    const uint32_t a = mode == MEAO_COMPOSITE_MULTIPLY ? unorm8_times(t >> 24, f) : t >> 24;
    return srgb_encode(srgb_decode(t & 255u) * f) | (srgb_encode(srgb_decode((t >> 8) & 255u) * f) << 8) |
           (srgb_encode(srgb_decode((t >> 16) & 255u) * f) << 16) | (a << 24);
}

__device__ __forceinline__ uint32_t composite_r11g11b10f(uint32_t t, float ao, int32_t mode)
{
    if (mode == MEAO_COMPOSITE_DEBUG) return f32_to_r11g11b10f(ao, ao, ao);
    const float f = composite_factor(ao, mode);
    return f32_to_r11g11b10f(ufloat_to_f32<6>(t & 0x7ffu) * f, ufloat_to_f32<6>((t >> 11) & 0x7ffu) * f, ufloat_to_f32<5>(t >> 22) * f);
}

__device__ __forceinline__ float4v composite_rgba32f(float4v t, float ao, int32_t mode)
{
    if (mode == MEAO_COMPOSITE_DEBUG) return float4v{ao, ao, ao, ao};
    const float f = composite_factor(ao, mode);
    return float4v{t.x * f, t.y * f, t.z * f, mode == MEAO_COMPOSITE_MULTIPLY ? t.w * f : t.w};
}

__device__ __forceinline__ uint8_t composite_gbuffer0_alpha(uint8_t a, float ao)
{
    return static_cast<uint8_t>(unorm8_times(a, composite_factor(ao, MEAO_COMPOSITE_AMBIENT_ONLY)));       // GBuffer0.a = occlusion
}

// Texels per 16-byte colour access.
template <int CFMT>
struct ColorGroup { static constexpr uint32_t kTexels = CFMT == MEAO_COLOR_RGBA32F ? 1u : 4u, kTexelBytes = 16u / kTexels; };

// Group gx of a row (texels kTexels * gx ...), vector form: every load of the lane is issued before the first use.  ao_at /
// color_at / g_at: the row's first texel, in texels of its surface from the frame base.
template <int AOFMT, int CFMT>
__device__ __forceinline__ void composite_format_group(const void *ao_base, void *color_base, void *gbuffer0_base, uint32_t ao_at,
                                                       uint32_t color_at, uint32_t g_at, int32_t mode, uint32_t gx)
{
    typedef AoTexel<AOFMT> AO;
    typedef typename AO::type ao_t;
    constexpr uint32_t T = ColorGroup<CFMT>::kTexels;
    const uint32_t x0 = gx * T;
    const ao_t *ap = at_byte_offset(static_cast<const ao_t *>(ao_base), (ao_at + x0) * static_cast<uint32_t>(sizeof(ao_t)));
    uint4v *cp = at_byte_offset(static_cast<uint4v *>(color_base), (color_at + x0) * ColorGroup<CFMT>::kTexelBytes);
    uint8_t *gp = at_byte_offset(static_cast<uint8_t *>(gbuffer0_base), (g_at + x0) * 4u);
    const bool ambient = mode == MEAO_COMPOSITE_AMBIENT_ONLY;
    uint4v raw = *cp;
    float aov[T];
    uint8_t ga[T] = {};
    if constexpr (T == 1) {
        const ao_t a1 = *ap;
        if (ambient) ga[0] = gp[3];
        aov[0] = AO::decode(a1);
    } else {
        const typename AO::type4 a4 = *reinterpret_cast<const typename AO::type4 *>(ap);
        if (ambient) {
#pragma unroll
            for (uint32_t e = 0; e < T; ++e) ga[e] = gp[4u * e + 3u];
        }
        aov[0] = AO::decode(a4.x); aov[1] = AO::decode(a4.y); aov[2] = AO::decode(a4.z); aov[3] = AO::decode(a4.w);
    }
    if constexpr (CFMT == MEAO_COLOR_RGBA32F) {
        raw = __builtin_bit_cast(uint4v, composite_rgba32f(__builtin_bit_cast(float4v, raw), aov[0], mode));
    } else if constexpr (CFMT == MEAO_COLOR_RGBA8) {
        raw.x = composite_rgba8(raw.x, aov[0], mode); raw.y = composite_rgba8(raw.y, aov[1], mode);
        raw.z = composite_rgba8(raw.z, aov[2], mode); raw.w = composite_rgba8(raw.w, aov[3], mode);
    } else if constexpr (CFMT == MEAO_COLOR_RGBA8_SRGB) {
        raw.x = composite_rgba8_srgb(raw.x, aov[0], mode); raw.y = composite_rgba8_srgb(raw.y, aov[1], mode);
        raw.z = composite_rgba8_srgb(raw.z, aov[2], mode); raw.w = composite_rgba8_srgb(raw.w, aov[3], mode);
    } else {
        raw.x = composite_r11g11b10f(raw.x, aov[0], mode); raw.y = composite_r11g11b10f(raw.y, aov[1], mode);
        raw.z = composite_r11g11b10f(raw.z, aov[2], mode); raw.w = composite_r11g11b10f(raw.w, aov[3], mode);
    }
    *cp = raw;
    if (ambient) {
#pragma unroll
        for (uint32_t e = 0; e < T; ++e) gp[4u * e + 3u] = composite_gbuffer0_alpha(ga[e], aov[e]);
    }
}

// Texel x of a row, scalar form: the widest accesses a surface without any alignment beyond its channel type allows (RGBA8 by
// and RGBA8_SRGB by bytes, RGBA32F and R11G11B10F by 32-bit words), with the results of the vector form.
template <int AOFMT, int CFMT>
__device__ __forceinline__ void composite_format_texel(const void *ao_base, void *color_base, void *gbuffer0_base, uint32_t ao_at,
                                                       uint32_t color_at, uint32_t g_at, int32_t mode, uint32_t x)
{
    typedef AoTexel<AOFMT> AO;
    typedef typename AO::type ao_t;
    const float ao = AO::decode(*at_byte_offset(static_cast<const ao_t *>(ao_base), (ao_at + x) * static_cast<uint32_t>(sizeof(ao_t))));
    const uint32_t color_byte = (color_at + x) * ColorGroup<CFMT>::kTexelBytes;
    if constexpr (CFMT == MEAO_COLOR_RGBA32F) {
        float *cp = at_byte_offset(static_cast<float *>(color_base), color_byte);
        const float4v t = composite_rgba32f(float4v{cp[0], cp[1], cp[2], cp[3]}, ao, mode);
        cp[0] = t.x; cp[1] = t.y; cp[2] = t.z; cp[3] = t.w;
    } else if constexpr (CFMT == MEAO_COLOR_RGBA8 || CFMT == MEAO_COLOR_RGBA8_SRGB) {
        uint8_t *cp = at_byte_offset(static_cast<uint8_t *>(color_base), color_byte);
        const uint32_t in = cp[0] | (uint32_t(cp[1]) << 8) | (uint32_t(cp[2]) << 16) | (uint32_t(cp[3]) << 24);
        const uint32_t t = CFMT == MEAO_COLOR_RGBA8 ? composite_rgba8(in, ao, mode) : composite_rgba8_srgb(in, ao, mode);
        cp[0] = static_cast<uint8_t>(t); cp[1] = static_cast<uint8_t>(t >> 8); cp[2] = static_cast<uint8_t>(t >> 16); cp[3] = static_cast<uint8_t>(t >> 24);
    } else {
        uint32_t *cp = at_byte_offset(static_cast<uint32_t *>(color_base), color_byte);
        *cp = composite_r11g11b10f(*cp, ao, mode);
    }
    if (mode == MEAO_COMPOSITE_AMBIENT_ONLY) {
        uint8_t *gp = at_byte_offset(static_cast<uint8_t *>(gbuffer0_base), (g_at + x) * 4u + 3u);
        *gp = composite_gbuffer0_alpha(*gp, ao);
    }
}

// The w texels of one row, dealt to `lanes` lanes: whole groups in the vector form where the surfaces are eligible, the last
// w mod kTexels texels -- or, on other surfaces, every texel -- in the scalar form.
template <int AOFMT, int CFMT>
__device__ __forceinline__ void composite_format_row(const void *ao_base, void *color_base, void *gbuffer0_base, uint32_t ao_at,
                                                     uint32_t color_at, uint32_t g_at, uint32_t w, bool vec, int32_t mode,
                                                     uint32_t lane, uint32_t lanes)
{
    constexpr uint32_t T = ColorGroup<CFMT>::kTexels;
    uint32_t done = 0;
    if (vec) {
        const uint32_t groups = w / T;
        for (uint32_t gx = lane; gx < groups; gx += lanes)
            composite_format_group<AOFMT, CFMT>(ao_base, color_base, gbuffer0_base, ao_at, color_at, g_at, mode, gx);
        done = groups * T;
    }
    for (uint32_t x = done + lane; x < w; x += lanes)
        composite_format_texel<AOFMT, CFMT>(ao_base, color_base, gbuffer0_base, ao_at, color_at, g_at, mode, x);
}

// Entry `frame` of the sized form's table (meao_composite_batch_extents).  Read through the constant address space, as
// composite_frame below reads the batched form's: 64-byte entries written by a copy ordered before the launch and never during
// it, so every field of a frame -- its extent, strides, lanes per row and form too -- is workgroup-uniform and sits in scalar registers.
__device__ __forceinline__ const CompositeSizedFrame &composite_sized_frame(const CompositeSizedFrame *table, uint32_t frame)
{
    typedef const __attribute__((address_space(4))) char *const_bytes;
    const const_bytes p = (const_bytes)table + static_cast<uint32_t>(sizeof(CompositeSizedFrame)) * frame;
    return *(const CompositeSizedFrame *)p;
}

// What the row forms deal: the launch's own surfaces, pitches and lanes per row, or -- kernel-uniform, the sized form -- those of
// frame blockIdx.y from its table entry.  Read behind the packed paths, which therefore do what they did.
struct CompositeRowFrame {
    const void *ao;
    void *color, *gbuffer0;
    CompositePitches p;
    uint32_t row_lanes_log2;
};
__device__ __forceinline__ CompositeRowFrame composite_row_frame(const CompositeArgs &a, const void *ao, void *color, void *gbuffer0)
{
    CompositeRowFrame r{ao, color, gbuffer0, a.pitch, static_cast<uint32_t>(a.row_lanes_log2)};
    if (a.sized != nullptr) {
        const CompositeSizedFrame &t = composite_sized_frame(a.sized, blockIdx.y);
        r.ao = t.ao; r.color = t.color; r.gbuffer0 = t.gbuffer0;
        r.p.ao = t.ao_stride; r.p.color = t.color_stride; r.p.gbuffer0 = t.gbuffer0_stride;
        r.p.w = t.w; r.p.h = t.h; r.p.vec = t.vec;
        r.row_lanes_log2 = static_cast<uint32_t>(t.row_lanes_log2);
    }
    return r;
}

// A frame in colour format CFMT: tightly packed = one row of `pixels` texels for the frame's workgroups, else rows as in the RGBA16F form.
template <int AOFMT, int CFMT>
__device__ __forceinline__ void composite_format_frame(const CompositeArgs &a, const void *ao, void *color, void *gbuffer0)
{
    if (!a.pitch.on) {
        composite_format_row<AOFMT, CFMT>(ao, color, gbuffer0, 0u, 0u, 0u, static_cast<uint32_t>(a.pixels), a.pitch.vec != 0, a.mode,
                                          blockIdx.x * kThreads + threadIdx.x, gridDim.x * kThreads);
        return;
    }
    const CompositeRowFrame r = composite_row_frame(a, ao, color, gbuffer0);
    const uint32_t lanes = 1u << r.row_lanes_log2, rows = static_cast<uint32_t>(kThreads) >> r.row_lanes_log2;
    for (uint32_t row = blockIdx.x * rows + (threadIdx.x >> r.row_lanes_log2); row < static_cast<uint32_t>(r.p.h); row += gridDim.x * rows)
        composite_format_row<AOFMT, CFMT>(r.ao, r.color, r.gbuffer0, __umul24(row, r.p.ao), __umul24(row, r.p.color),
                                          __umul24(row, r.p.gbuffer0), static_cast<uint32_t>(r.p.w), r.p.vec != 0, a.mode,
                                          threadIdx.x & (lanes - 1u), lanes);
}

// Entry `frame` of the batched form's table (meao_composite_batch).  Read through the constant address space, as frame_block
// reads the FrameArgs table: written by a copy ordered before the launch and never during it, so the three origins are
// workgroup-uniform scalar loads.
__device__ __forceinline__ const CompositeFrame &composite_frame(const CompositeFrame *table, uint32_t frame)
{
    typedef const __attribute__((address_space(4))) char *const_bytes;
    const const_bytes p = (const_bytes)table + static_cast<uint32_t>(sizeof(CompositeFrame)) * frame;
    return *(const CompositeFrame *)p;
}

}  // namespace
}  // namespace meao
