"""NumPy model of the composite into RGBA32F, RGBA8 and R11G11B10F colour targets (meao_composite_format), written from the
canonical reading in include/meao.h with integer bit operations -- not from the kernel.

Operands are widened to f32, one f32 multiply is done per channel (f = ao in MULTIPLY, keep = 1 - (1 - ao) in AMBIENT_ONLY), and
the result is rounded to the target format.  Test infrastructure: tests/test_color_format_model.py checks the model itself,
tests/test_composite_formats_gpu.py the library against it."""
import numpy as np

RGBA16F, RGBA32F, RGBA8, R11G11B10F = 0, 1, 2, 3
MULTIPLY, AMBIENT_ONLY, DEBUG = 0, 1, 2
TEXEL_BYTES = {RGBA16F: 8, RGBA32F: 16, RGBA8: 4, R11G11B10F: 4}
AO_R8, AO_F16 = 0, 1


# ---- unsigned small floats: 5-bit exponent of bias 15, M mantissa bits (6 for R and G, 5 for B)

def dec(code, M):
    """code -> float32, exact: e = 0: m * 2^(-14 - M); 0 < e < 31: (1 + m / 2^M) * 2^(e - 15); e = 31: m = 0 +inf, else NaN."""
    code = np.asarray(code, np.int64)
    e, m = code >> M, code & ((1 << M) - 1)
    sub = np.ldexp(m.astype(np.float64), -14 - M)
    nor = np.ldexp(((1 << M) + m).astype(np.float64), (e - 15 - M).astype(np.int32))
    top = np.where(m == 0, np.inf, np.nan)
    return np.where(e == 0, sub, np.where(e == 31, top, nor)).astype(np.float32)


def enc(x, M):
    """float32 -> code: NaN of either sign -> all ones, anything with the sign bit set -> 0, +inf -> e = 31 m = 0, otherwise round
    to nearest even with gradual underflow; what rounds past the largest finite code becomes +inf."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    inf = 31 << M
    e, frac = (u >> 23) & 0xff, u & 0x7fffff
    sig = np.where(e > 0, frac | 0x800000, frac)                 # value = sig * 2^(max(e, 1) - 150)
    target = np.maximum(e - 127, -14)                            # the result is a multiple of 2^(target - M)
    drop = np.minimum(target - M - (np.maximum(e, 1) - 150), 40)  # >= 23 - M low bits go; 40 and more leave nothing either way
    q, rest, half = sig >> drop, sig & ((1 << drop) - 1), 1 << (drop - 1)
    q = q + ((rest > half) | ((rest == half) & ((q & 1) == 1)))
    code = np.where(e - 127 >= -14, ((e - 127 + 14) << M) + q, q)    # q carries the leading one of a normal number
    code = np.minimum(code, inf)
    code = np.where((u >> 31) == 1, 0, code)
    code = np.where((u & 0x7fffffff) > 0x7f800000, inf | ((1 << M) - 1), code)
    return code.astype(np.uint32)


def unpack_r11g11b10f(t):
    t = np.asarray(t, np.uint32)
    return dec(t & 0x7ff, 6), dec((t >> 11) & 0x7ff, 6), dec(t >> 22, 5)


def pack_r11g11b10f(r, g, b):
    return (enc(r, 6) | (enc(g, 6) << 11) | (enc(b, 5) << 22)).astype(np.uint32)


# ---- UNORM8: the conversions of the AO stores and of GBuffer0.a

def unorm8_to_f32(code):
    return np.asarray(code).astype(np.float32) / np.float32(255.0)          # correctly rounded


def f32_to_unorm8(x):
    """saturate with NaN -> 0, x 255 and + 0.5 as two f32 roundings, truncate."""
    x = np.asarray(x, np.float32)
    s = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    s = (s * np.float32(255.0)).astype(np.float32)
    s = (s + np.float32(0.5)).astype(np.float32)
    return s.astype(np.uint32)


def ao_to_f32(ao, ao_format):
    """AO texels as stored (uint8 codes / f16 bit patterns or float16) -> float32."""
    ao = np.asarray(ao)
    if ao_format == AO_R8:
        return unorm8_to_f32(ao)
    return (ao if ao.dtype == np.float16 else ao.view(np.float16)).astype(np.float32)


def factor(ao32, mode):
    if mode == MULTIPLY:
        return ao32
    occ = (np.float32(1) - ao32).astype(np.float32)
    return (np.float32(1) - occ).astype(np.float32)


# ---- the composite

def composite(ao, ao_format, color, color_format, mode, gbuffer0=None):
    """-> (color', gbuffer0').  color: (H, W, 4) float32 (RGBA32F) / uint8 (RGBA8), (H, W) uint32 (R11G11B10F); gbuffer0
    (H, W, 4) uint8 or None, touched in AMBIENT_ONLY only.  Inputs are not modified."""
    with np.errstate(all="ignore"):
        a = ao_to_f32(ao, ao_format)
        f = factor(a, mode)
        if color_format == RGBA32F:
            c = np.array(color, np.float32)
            if mode == DEBUG:
                c[...] = a[..., None]
            else:
                k = 4 if mode == MULTIPLY else 3
                c[..., :k] = (c[..., :k] * f[..., None]).astype(np.float32)
        elif color_format == RGBA8:
            c = np.array(color, np.uint8)
            if mode == DEBUG:
                c[...] = f32_to_unorm8(a)[..., None]
            else:
                k = 4 if mode == MULTIPLY else 3
                c[..., :k] = f32_to_unorm8((unorm8_to_f32(c[..., :k]) * f[..., None]).astype(np.float32))
        elif color_format == R11G11B10F:
            if mode == DEBUG:
                c = pack_r11g11b10f(a, a, a)
            else:
                r, g, b = unpack_r11g11b10f(color)
                c = pack_r11g11b10f((r * f).astype(np.float32), (g * f).astype(np.float32), (b * f).astype(np.float32))
        else:
            raise ValueError(color_format)
        g0 = None if gbuffer0 is None else np.array(gbuffer0, np.uint8)
        if mode == AMBIENT_ONLY and g0 is not None:
            g0[..., 3] = f32_to_unorm8((unorm8_to_f32(g0[..., 3]) * f).astype(np.float32))
    return c, g0
