"""The rule behind the white-tile shortcut of the full-resolution upsample (meao_dev_upsample.hpp, "white tile"), checked on the
CPU oracle alone: a 64 x 64 tile whose clamp-addressed 38 x 38 `combined1` window is all code 255 has an all-255 `result` tile --
whatever the depths are, as long as no hi-res depth texel of the tile is NaN (the reference stores 0 there: such a lane is not
clean and the library's tile takes the normal path).

Beyond the default context (second half of the file): the same for 64 x 32 tiles (38 x 22 window, rows [16 ty - 3, 16 ty + 18]) and
for one level (the window is `occlusion1`), on all-sky, half-sky, radial, constant and occluder frames under both Z conventions, f32
and UNORM16 depth, both f16 roundings, 1..4 levels, both sides of the three edges of the exact-division range and the far-outside
parameter values.  White-tile counts at 4 levels, f32, RTZ (64 x 64 / 64 x 32): all-sky 30 / 60 (RTNE: 0), half-sky 10 / 20 (the
plane's tiles: the sky half's low-res AO is not white), radial 2 / 4, constant 30 / 60 (UNORM16 too).  The last three tests evaluate
what the GPU tests of tests/test_white_tiles_window_gpu.py assume of their frames (set MEAO_PRINT_BANDS=1 and run with -s for the
table of narrowest bands)."""
import dataclasses
import os

import numpy as np
import pytest

from miniengineao_amd import synth
from tests import helpers as H
from tests import white_tiles as WT


def white_and_broken(oracle, depth, s):
    r = oracle.run(depth, s)
    tiles = WT.white_tiles(r["combined1"], s.width, s.height)
    return tiles, [t for t in tiles if (WT.result_tile(r["result"], *t) != 255).any()]


def test_s2_frames(oracle):
    s = H.settings(oracle, 1024, 576)
    counts = []
    for seed in (1, 2, 3):
        tiles, broken = white_and_broken(oracle, synth.make("S2", 1024, 576, seed=seed), s)
        assert not broken, (seed, broken)
        counts.append(len(tiles))
    assert max(counts) > 0, "no S2 frame has a white tile: the test checks nothing"


def test_atrium(oracle):
    cam = synth.SPONZA_CAMERA
    s = H.settings(oracle, 960, 540, cam=cam)
    tiles, broken = white_and_broken(oracle, synth.atrium(960, 540), s)
    assert not broken, broken
    assert tiles, "the atrium has no white tile: the test checks nothing"


def test_white_frames_of_the_gpu_test(oracle):
    s = H.settings(oracle, WT.W, WT.H)
    for d in (WT.flat_frame(), WT.apron_frame()):
        tiles, broken = white_and_broken(oracle, d, s)
        assert tiles and not broken


def test_a_nan_on_an_odd_texel_of_a_white_tile_is_the_one_exception(oracle):
    """Frame 3 of tests/test_white_tiles_gpu.py: the window stays white (no level is made of an odd texel), the reference stores 0
    at the NaN texel and 255 everywhere else -- why an unclean lane must send the tile down the normal path."""
    s = H.settings(oracle, WT.W, WT.H)
    r = oracle.run(WT.texel_frame(WT.ODD_TEXEL, np.float32(np.nan)), s)
    assert (r["combined1"] == 255).all()
    assert np.argwhere(r["result"] != 255).tolist() == [list(WT.ODD_TEXEL)] and r["result"][WT.ODD_TEXEL] == 0


@pytest.mark.parametrize("name", sorted(WT.ODD_VALUES))
def test_other_hostile_values_on_that_texel_keep_the_tile_white(oracle, name):
    s = H.settings(oracle, WT.W, WT.H)
    r = oracle.run(WT.texel_frame(WT.ODD_TEXEL, WT.ODD_VALUES[name]), s)
    assert (r["combined1"] == 255).all() and (r["result"] == 255).all()


# ---- the rule beyond the default context: frames and settings the shortcut meets in the field, both tile heights

CONV_CAMERA = dataclasses.replace(synth.DEFAULT_CAMERA, reversed_z=False)
CAMERAS = {"revz": synth.DEFAULT_CAMERA, "convz": CONV_CAMERA}
# white 64 x 64 tiles at 4 levels, f32 depth, RTZ -- the same under both Z conventions (the frames are built from Linear01 depth)
WHITE_COUNTS = {"sky": 30, "half_sky": 10, "radial": 2, "flat": 30}
EDGE_TABLE = {"upsample_low": (-13.245319, -13.245320), "upsample_high": (6.0205998, 6.0206003), "noise_high": (9.030899, 9.030900)}


def field_frames(cam):
    flat = WT.flat_frame() if cam.reversed_z else synth.linear01_to_raw(np.full((WT.H, WT.W), 0.1), cam)
    return {"sky": WT.sky_frame(cam.reversed_z), "half_sky": WT.half_sky_frame(cam), "radial": synth.radial_gradient(WT.W, WT.H, cam),
            "flat": flat, "occluders": WT.sky_and_flat_occluders(cam)}


def rule_holds(oracle, depth, s):
    """Asserts the rule for both tile heights; returns the white-tile counts (64 x 64, 64 x 32) and the oracle's outputs."""
    r = oracle.run(oracle.encode_depth(depth, s.depth_format), s)
    counts = []
    for tile_h in (64, 32):
        tiles, broken = WT.broken_tiles(r, s, tile_h)
        assert not broken, (tile_h, broken)
        counts.append(len(tiles))
    return counts, r


def test_the_generalised_predicate_is_the_old_one_for_64_x_64_tiles(oracle):
    s = H.settings(oracle, WT.W, WT.H)
    for d in (WT.apron_frame(), WT.leak_frame(), synth.make("S2", WT.W, WT.H, seed=3)):
        r = oracle.run(d, s)
        assert WT.white_tiles_h(r["combined1"], WT.W, WT.H) == WT.white_tiles(r["combined1"], WT.W, WT.H)


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("name", ["sky", "half_sky", "radial", "flat", "occluders"])
def test_field_frames_formats_roundings_and_levels(oracle, name, cam):
    depth = field_frames(CAMERAS[cam])[name]
    for fmt in (oracle.DEPTH_F32, oracle.DEPTH_UNORM16):
        for rounding in (oracle.F16_RTZ, oracle.F16_RTNE):
            for levels in (1, 2, 3, 4):
                s = H.settings(oracle, WT.W, WT.H, cam=CAMERAS[cam], depth_format=fmt, f16_rounding=rounding, num_levels=levels)
                counts, r = rule_holds(oracle, depth, s)
                if levels == 4 and rounding == oracle.F16_RTZ and name in WHITE_COUNTS and (fmt == oracle.DEPTH_F32 or name in ("sky", "flat")):
                    assert counts == [WHITE_COUNTS[name], 2 * WHITE_COUNTS[name] if name != "radial" else 4], (fmt, counts)
                if name == "sky" and rounding == oracle.F16_RTNE:
                    assert counts == [0, 0]         # under RTNE the sky's low-res AO is not code 255: no sky tile is white
                if name == "occluders" and levels == 4 and rounding == oracle.F16_RTZ and fmt == oracle.DEPTH_F32:
                    white = WT.white_tiles_h(WT.low_ao(r, s), WT.W, WT.H)
                    assert (4, 3) in white and (4, 4) in white, white      # from-raw tiles inside the flat block
                    assert not [t for t in white if t[0] < 3 and t[1] < 3], white      # none in the sky block (WT.sky_and_flat_occluders)


def test_exact_range_edges_of_the_oracle_are_the_documented_ones(oracle):
    edges = WT.oracle_exact_range_edges(oracle, H.settings(oracle, WT.W, WT.H))
    for k, (inside, outside) in EDGE_TABLE.items():
        assert (np.float32(edges[k][1]), np.float32(edges[k][2])) == (np.float32(inside), np.float32(outside)), (k, edges[k])


@pytest.mark.parametrize("cam", sorted(CAMERAS))
def test_parameter_edges_and_far_outside_values(oracle, cam):
    """Both sides of the three edges of the exact-division range, and helpers.FAR_OUTSIDE: the rule is one of the reference, not of
    the range the library's proof of it leans on."""
    frames = field_frames(CAMERAS[cam])
    base = H.settings(oracle, WT.W, WT.H, cam=CAMERAS[cam])
    values = [(f, v) for f, inside, outside in WT.oracle_exact_range_edges(oracle, base).values() for v in (inside, outside)]
    values += [(f, v) for f, vs in H.FAR_OUTSIDE.items() for v in vs]
    white = 0
    for field, v in values:
        s = dataclasses.replace(base, **{field: v})
        for name, depth in frames.items():
            counts, r = rule_holds(oracle, depth, s)
            white += counts[0]
            if name == "half_sky" and field == "upsample_tolerance" and v == np.float32(6.0205998):
                assert counts[0] == 10 and int((r["result"] != 255).sum()) == 71040      # non-white texels NEXT to the white tiles
    assert white > 0


# ---- what the GPU tests of tests/test_white_tiles_window_gpu.py assume of their frames, evaluated here without a GPU

@pytest.mark.parametrize("tile_h", [64, 32])
def test_window_plan(oracle, tile_h, capsys):
    with capsys.disabled():
        WT.check_window_plan(oracle, tile_h, log=print if os.environ.get("MEAO_PRINT_BANDS") else None)


@pytest.mark.parametrize("tile_h", [64, 32])
def test_nan_frames_visit_every_position_and_leave_the_window_white(oracle, tile_h):
    WT.check_nan_frames(oracle, tile_h)


@pytest.mark.parametrize("tile_h", [64, 32])
def test_partial_row_plan_and_nan_frames(oracle, tile_h):
    WT.check_partial_plan(oracle, tile_h)
    WT.check_partial_nan_frames(oracle, tile_h)


def test_partial_row_tiles_are_white_only_with_one_or_two_levels(oracle):
    """Why the partial-row frames run with two levels: the constant plane at 384 x 312."""
    for levels, white in ((1, 30), (2, 30), (3, 12), (4, 12)):
        s = H.settings(oracle, WT.W, WT.PARTIAL_H, num_levels=levels)
        counts, _ = rule_holds(oracle, WT.flat_frame(WT.W, WT.PARTIAL_H), s)
        assert counts[0] == white, (levels, counts)


def test_hostile_kinds_that_show_on_a_white_tile(oracle):
    assert WT.hostile_kinds_that_show(oracle) == ["nan"]
