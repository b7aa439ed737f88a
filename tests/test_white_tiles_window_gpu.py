"""The window test and the clean-lane test of the white-tile shortcut (meao_dev_upsample.hpp: quad_white, s_white, the ballot) on every
side, wave and lane position, bit for bit against the oracle, for 64 x 64 and 64 x 32 tiles.

Frames (tests/white_tiles.py window_plan): the constant plane with ONE 4 x 4 block of raw depth 0.1, placed so that one from-raw tile
sees non-white low-res AO only in chosen lines of its window while its result tile changes.  What each frame is for is asserted on
the oracle by WT.check_window_plan -- here, and without a GPU in tests/test_white_tile_rule.py::test_window_plan.

  sides     left / right / top / bottom: darkness only in the two outermost lines of that side, for a tile of an interior tile row, of
            tile row 0 (top apron clamp-addressed: bottom, left, right) and of the last full tile row (top, left, right).
            Not reachable: 64 x 32 tiles, last tile row, top -- a block that would darken window rows 0..1 stands so near the
            frame's bottom edge that the clamped lines 18..21 darken too (all 30 369 placements of the block searched); the nearest
            frame is kept: rows 1..2, columns 2..3.
  corners   all four, for both windows: darkness within 3 lines of both adjacent sides (rows / columns 1..2 or 35..36 [19..20]).
  sweeps    the block slid along the left apron (rows) and the top apron (columns) of the interior tile, 32 frames each (18 for
            the 22 rows).  Every line of the window is hit by a frame whose darkness lies in at most two bands of two adjacent lines
            -- except lines 16..21 of a 38-line axis: the darkness of a block comes in three bands 8 lines apart, and for those lines
            all three lie inside the window whichever band the line is in (4 x 4 and 8 x 8 blocks of 0.1, 0.0975 and 0.095
            searched over every even placement around a tile).  They are hit by three bands of two lines, and the check says so.
  partial   tile (2, 4) [(2, 9)] of the partial last tile row at 384 x 312 with TWO levels (WT.partial_plan; with 3 or 4 levels the
            reference's low-res AO is not code 255 from tile row 2 down at this size and no tile of that row is ever white; with
            1 or 2 levels the constant plane is white in all 30 tiles).  Such a tile is interior but not from-raw: it fills its
            window from the buffer, tests it there, and its white store loop masks the rows past the frame.  Left, right and top
            sides, the two top corners, a sweep down the left apron that darkens every window row, and NaNs at every wave and
            pass with rows inside the frame -- through surfaces with eight guard rows below the frame (packed, the plain kernels,
            and pitched), which must stay untouched.

The narrowest bands per line (oracle; identical for rows of the 38-row window and for columns of both windows):
   0 [0,1]   1 [0,1]   2 [1,2]   3 [2,3]   4 [4,5]   5 [4,5]   6 [5,6]   7 [6,7]   8 [0][7,8]   9 [1,2][9,10]   10 [1,2][9,10]
  11 [2,3][10,11]   12 [3,4][11,12]   13 [4,5][12,13]   14 [5,6][13,14]   15 [6,7][14,15]   16 [0][7,8][15,16]
  17 [8,9][16,17][24,25]   18 [9,10][17,18][25,26]   19 [10,11][18,19][26,27]   20 [4,5][12,13][20,21]   21 [21,22][29,30][37]
  22 [22,23][30,31]   23 [22,23][30,31]   24 [23,24][31,32]   25 [24,25][32,33]   26 [25,26][33,34]   27 [26,27][34,35]
  28 [27,28][35,36]   29 [29,30][37]   30 [30,31]   31 [30,31]   32 [31,32]   33 [32,33]   34 [34,35]   35 [34,35]   36 [35,36] (rows:
  [36,37])   37 [36,37]
rows of the 22-row window:  0 [0,1]  1 [0,1]  2 [1,2]  3 [2,3]  4 [4,5]  5 [4,5]  6 [5,6]  7 [6,7]  8 [0][7,8]  9 [8,9][16,17]
  10 [9,10][17,18]  11 [3,4][11,12]  12 [3,4][11,12]  13 [13,14][21]  14 [14,15]  15 [14,15]  16 [15,16]  17 [16,17]  18 [18,19]
  19 [18,19]  20 [20,21]  21 [20,21]
(Window items are dealt to waves in row order, 64 items = 6.4 rows a wave: single bands in rows 0..5 and 32..37 are seen by ONE wave
of the 64 x 64 tile -- wave 0, and wave 1 in its second round; the single bands of rows 14..21 of the 22-row window by wave 2 or 3
alone.  In the 38-row window waves 2 and 3 never see darkness alone: their rows come with a band 8 lines away.)

Unclean lanes: WT.nan_frames -- one NaN per from-raw tile of the constant plane, never on a level texel, visiting every (wave, pass,
row of the pair, odd-odd / odd-even / even-odd) with two columns of the lane's quad each; the oracle's low-res AO stays all 255 and
its result is 0 at exactly the NaN texels (WT.check_nan_frames).  Of the kinds of helpers.hostile_frame only NaN shows in the
oracle's result on such a texel (WT.hostile_kinds_that_show), so NaN is the only kind here."""
import numpy as np
import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import white_tiles as WT

pytestmark = pytest.mark.gpu

TILES = {64: {L.DEBUG_FINAL_SMALL_MAX_TILES: 0}, 32: None}       # tile height -> debug overrides (calls this small take 64 x 32 tiles)


def same(got, want, what):
    assert np.array_equal(got, want), H.diff_report(what, got, want) + " " + str(where(got, want))


def where(got, want):
    """The first differing texel as tile / wave / pass of both tile heights (meao_dev_upsample.hpp lane layout)."""
    y, x = np.argwhere(got != want)[0]
    return {h: WT.lane_position(int(y), int(x), h) for h in (64, 32)}


@pytest.fixture(scope="module")
def plans(oracle):
    """tile height -> (Settings, {group: [(spot, depth, oracle outputs)]}); computed once, never modified."""
    s = H.settings(oracle, WT.W, WT.H)
    out = {}
    for tile_h in TILES:
        WT.check_window_plan(oracle, tile_h)
        out[tile_h] = {g: [(sp,) + WT.spot_view(oracle, s, sp, tile_h)[:2] for sp in spots] for g, spots in WT.window_plan(tile_h).items()}
    return s, out


@pytest.mark.parametrize("tile_h", sorted(TILES))
@pytest.mark.parametrize("group", ["sides", "corners", "row_sweep", "col_sweep"])
def test_block_frames(plans, group, tile_h):
    """One batch per group: every frame's whole result and combined1 against the oracle."""
    s, plan = plans
    frames = plan[tile_h][group]
    ao = H.component(s, max_batch=len(frames), debug=TILES[tile_h])
    try:
        got = ao.render_batch([d for _, d, _ in frames])
        assert ao.hostile_frames() == 0
        for f, (spot, _, want) in enumerate(frames):
            same(got[f], want["result"], (group, tile_h, spot["at"]))
            same(ao.debug_buffer(14, frame=f), want["combined1"], ("combined1", spot["at"]))
    finally:
        ao.close()


@pytest.mark.parametrize("tile_h", sorted(TILES))
@pytest.mark.parametrize("per_frame", [False, True], ids=["shared", "per_frame_params"])
def test_the_white_decision_follows_the_frame_index(plans, oracle, per_frame, tile_h):
    """white, block, white: the same tile is white in frames 0 and 2 and not in frame 1."""
    s, plan = plans
    spot, block, want_block = plan[tile_h]["sides"][0]
    flat = WT.flat_frame()
    want_flat = oracle.run(flat, s)
    assert WT.window_white_h(want_flat["combined1"], *spot["tile"], tile_h) and not WT.window_white_h(want_block["combined1"], *spot["tile"], tile_h)
    ao = H.component(s, max_batch=3, debug=TILES[tile_h])
    try:
        got = ao.render_batch([flat, block, flat], params=[FrameParams()] * 3 if per_frame else None)
        for f, want in enumerate((want_flat, want_block, want_flat)):
            same(got[f], want["result"], (f, per_frame))
    finally:
        ao.close()


@pytest.mark.parametrize("tile_h", sorted(TILES))
def test_a_nan_at_every_lane_position_of_white_tiles(oracle, tile_h):
    frames = WT.check_nan_frames(oracle, tile_h)
    s = H.settings(oracle, WT.W, WT.H)
    ao = H.component(s, max_batch=len(frames), debug=TILES[tile_h])
    try:
        got = ao.render_batch([d for d, _ in frames])
        assert ao.hostile_frames() == 0                  # the exact-reciprocal instance ran: the one that has the shortcut
        for f, (_, want) in enumerate(frames):
            same(got[f], want["result"], ("nan", tile_h, f))
    finally:
        ao.close()


# ---- the partial last tile row (384 x 312, two levels): window-first tiles whose white stores are masked

def run_on_guarded_surfaces(s, depths, debug, pitch):
    """The frames through execute_tensors on surfaces with 8 guard rows below the frame (and pitch - width guard columns);
    returns the results after asserting that every guard texel kept its fill."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    n, h, w = len(depths), s.height, s.width
    dsurf = torch.full((n, h + 8, pitch), 0.5, dtype=torch.float32, device=dev)
    osurf = torch.full((n, h + 8, pitch), 7, dtype=torch.uint8, device=dev)
    for f, d in enumerate(depths):
        dsurf[f, :h, :w] = torch.from_numpy(np.array(d)).to(dev)
    ao = H.component(s, max_batch=n, debug=debug)
    try:
        ao.execute_tensors(dsurf[:, :h, :w], osurf[:, :h, :w])
        torch.cuda.synchronize(dev)
        assert ao.hostile_frames() == 0
        low = [ao.debug_buffer(14, frame=f) for f in range(n)]
    finally:
        ao.close()
    got = osurf.cpu().numpy()
    assert (got[:, h:, :] == 7).all() and (got[:, :, w:] == 7).all(), "texels behind the surface were written"
    return [got[f, :h, :w] for f in range(n)], low


@pytest.mark.parametrize("tile_h", sorted(TILES))
@pytest.mark.parametrize("pitch", [WT.W, WT.W + 16], ids=["packed", "pitched"])
@pytest.mark.parametrize("group", ["sides", "row_sweep", "nans"])
def test_partial_last_tile_row(oracle, group, pitch, tile_h):
    s = WT.partial_settings(oracle)
    flat = WT.flat_frame(WT.W, WT.PARTIAL_H)
    if group == "nans":
        frames = [("nan", d, want) for d, want in WT.check_partial_nan_frames(oracle, tile_h)]
    else:
        WT.check_partial_plan(oracle, tile_h)
        frames = [(sp["at"],) + WT.spot_view(oracle, s, sp, tile_h)[:2] for sp in WT.partial_plan(tile_h)[group]]
    frames.append(("flat", flat, oracle.run(flat, s)))              # every tile white, the partial row too
    got, low = run_on_guarded_surfaces(s, [d for _, d, _ in frames], TILES[tile_h], pitch)
    for f, (what, _, want) in enumerate(frames):
        same(got[f], want["result"], (group, tile_h, pitch, what))
        same(low[f], want["combined1"], ("combined1", what))
