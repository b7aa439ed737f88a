"""Frames and the oracle-side rule of the white-tile shortcut of the full-resolution upsample (meao_dev_upsample.hpp, "white
tile"), shared by tests/test_white_tile_rule.py (CPU), tests/test_white_tiles_gpu.py and tests/white_tiles_variant_check.py.

The rule: a 64 x 64 tile of the result whose low-res AO window -- the 38 x 38 `combined1` texels [32 tx - 3, 32 tx + 34] x
[32 ty - 3, 32 ty + 34], clamp-addressed -- is all code 255 is all 255 itself, unless a hi-res depth texel of the tile is not
clean (NaN: the reference stores 0 there)."""
import numpy as np

W, H = 384, 320                     # 6 x 5 tiles of 64 x 64; the from-raw tiles are columns 1..4 (meao_dev_upsample.hpp ups_tile_from_raw)
TILE = 64
FLAT = np.float32(0.09)             # raw depth (reversed Z) of the constant frame
DARK = np.float32(0.07)
DARK_BLOCK = (slice(118, 124), slice(182, 188))      # rows y 118..123, columns x 182..187
NEAR = np.float32(0.2)
LEAK_BLOCK = (slice(140, 148), slice(160, 168))        # rows y 140..147, columns x 160..167
ODD_TEXEL = (97, 99)                # (y, x): odd row, odd column, inside from-raw tile (1, 1) -- no level is made of it
LEVEL_TEXEL = (96, 98)              # (y, x): even row, even column -- a LowDepth1 texel: the frame takes the IEEE instance
ODD_VALUES = {"pinf": np.float32(np.inf), "neg": np.float32(-1.0), "zero": np.float32(0.0), "one": np.float32(1.0)}


def flat_frame(w=W, h=H):
    return np.full((h, w), FLAT, np.float32)


def apron_frame():
    d = flat_frame()
    d[DARK_BLOCK] = DARK
    return d


def texel_frame(at, value):
    d = flat_frame()
    d[at] = value
    return d


def leak_frame():
    """A nearer 8 x 8 block in tile (2, 2): the plane around it darkens AT THE PLANE'S DEPTH (the blur keeps such taps), and for the
    tiles next to it that darkness lies only in the apron of their window -- yet reaches result texels inside them."""
    d = flat_frame()
    d[LEAK_BLOCK] = NEAR
    return d


def linear_z_of_constant(raw, cam):
    """z = Linearize(raw) * far for one raw depth value that is no sky texel, as the oracle evaluates it:
    1 / fmaf(zp.x, raw, zp.y), the fused multiply-add rounded once (exact rational arithmetic here), far_clip a power of two."""
    from fractions import Fraction
    fpn = np.float32(cam.far) / np.float32(cam.near)
    zp0, zp1 = (fpn - np.float32(1), np.float32(1)) if cam.reversed_z else (np.float32(1) - fpn, fpn)
    exact = Fraction(float(zp0)) * Fraction(float(np.float32(raw))) + Fraction(float(zp1))
    c = np.float32(float(exact))
    cands = [c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))]
    den = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
    dist = np.float32(1) / den
    assert dist < 1 and float(cam.far) == 2.0 ** round(np.log2(cam.far))
    return np.float32(dist * np.float32(cam.far))


from miniengineao_amd.synth import interior_white, white_tiles, window_white      # noqa: E402  (the rule lives next to the frames' generators)
from miniengineao_amd.synth import white_tile_map as tile_map                     # noqa: E402


def result_tile(result, tx, ty):
    return result[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
