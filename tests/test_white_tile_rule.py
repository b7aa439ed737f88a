"""The rule behind the white-tile shortcut of the full-resolution upsample (meao_dev_upsample.hpp, "white tile"), checked on the
CPU oracle alone: a 64 x 64 tile whose clamp-addressed 38 x 38 `combined1` window is all code 255 has an all-255 `result` tile --
whatever the depths are, as long as no hi-res depth texel of the tile is NaN (the reference stores 0 there: such a lane is not
clean and the library's tile takes the normal path)."""
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
