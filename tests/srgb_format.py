"""NumPy model of the composite into sRGB colour targets (MEAO_COLOR_RGBA8_SRGB), written from the canonical reading in
include/meao.h -- not from the kernel, and not from the committed table include: both tables are computed here with mpmath.

r, g, b are sRGB-encoded UNORM8 and blended in linear light: c' = enc(D[c] * f), one f32 multiply per channel.  Alpha is linear
UNORM8 and moves as in RGBA8; GBuffer0 as in every colour format (the conversions of tests/color_formats.py).
  D[k], k = 0..255: the f32 nearest to lin(k / 255);  T[k], k = 1..255: the smallest f32 >= lin((k - 0.5) / 255);
  lin(s) = s / 12.92 for s <= 0.04045, ((s + 0.055) / 1.055)^2.4 otherwise;  enc(x) = the number of k with x >= T[k], NaN -> 0.
Test infrastructure: tests/test_srgb_model.py checks the model itself, tests/test_composite_srgb_gpu.py the library against it."""
import functools

import mpmath
import numpy as np

from tests import color_formats as CF

RGBA8_SRGB = 5
MULTIPLY, AMBIENT_ONLY, DEBUG = CF.MULTIPLY, CF.AMBIENT_ONLY, CF.DEBUG
AO_R8, AO_F16 = CF.AO_R8, CF.AO_F16
BITS = 200


def lin(s):
    """sRGB-encoded s in [0, 1] -> linear light, in the working precision of mpmath."""
    s = mpmath.mpf(s)
    if s <= mpmath.mpf("0.04045"):
        return s / mpmath.mpf("12.92")
    return ((s + mpmath.mpf("0.055")) / mpmath.mpf("1.055")) ** mpmath.mpf("2.4")


def decode_point(k):
    return lin(mpmath.mpf(k) / 255)


def boundary(k):
    """The linear-light value at which code k begins: half a code below k in the encoded domain."""
    return lin((mpmath.mpf(k) - mpmath.mpf("0.5")) / 255)


def _neighbours(v):
    """The f32 values around the real v: the nearest double rounded to f32, and one step either way."""
    c = np.float32(float(v))
    return [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]


def _nearest_f32(v):
    return min(_neighbours(v), key=lambda c: abs(mpmath.mpf(float(c)) - v))


def _ceil_f32(v):
    return min(c for c in _neighbours(v) if mpmath.mpf(float(c)) >= v)


@functools.lru_cache(maxsize=None)
def tables():
    """-> (D float32 [256], T float32 [255]: T[i] is the threshold of code i + 1).  Computed once; treat as read-only."""
    with mpmath.workprec(BITS):
        d = np.array([np.float32(0)] + [_nearest_f32(decode_point(k)) for k in range(1, 256)], np.float32)
        t = np.array([_ceil_f32(boundary(k)) for k in range(1, 256)], np.float32)
    d.setflags(write=False)
    t.setflags(write=False)
    return d, t


def dec(code):
    return tables()[0][np.asarray(code, np.int64)]


def enc(x):
    """float32 -> code: the number of thresholds at or below x; NaN of either sign -> 0."""
    x = np.asarray(x, np.float32)
    k = np.searchsorted(tables()[1], x, side="right")
    return np.where(np.isnan(x), 0, k).astype(np.uint8)


def composite(ao, ao_format, color, color_format, mode, gbuffer0=None):
    """-> (color', gbuffer0'), the signature of color_formats.composite.  color: (H, W, 4) uint8; gbuffer0 (H, W, 4) uint8 or None,
    touched in AMBIENT_ONLY only.  Inputs are not modified."""
    if color_format != RGBA8_SRGB:
        raise ValueError(color_format)
    with np.errstate(all="ignore"):
        a = CF.ao_to_f32(ao, ao_format)
        f = CF.factor(a, mode)
        c = np.array(color, np.uint8)
        if mode == DEBUG:
            c[..., :3] = enc(a)[..., None]
            c[..., 3] = CF.f32_to_unorm8(a)
        else:
            c[..., :3] = enc((dec(c[..., :3]) * f[..., None]).astype(np.float32))
            if mode == MULTIPLY:
                c[..., 3] = CF.f32_to_unorm8((CF.unorm8_to_f32(c[..., 3]) * f).astype(np.float32))
        g0 = None if gbuffer0 is None else np.array(gbuffer0, np.uint8)
        if mode == AMBIENT_ONLY and g0 is not None:
            g0[..., 3] = CF.f32_to_unorm8((CF.unorm8_to_f32(g0[..., 3]) * f).astype(np.float32))
    return c, g0
