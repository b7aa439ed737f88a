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


}  // namespace
}  // namespace meao
