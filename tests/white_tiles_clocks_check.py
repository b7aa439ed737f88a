"""Which path the full-resolution tiles take, read from the phase stamps of the `clocks` variant library (MEAO_LIB_PATH; built
with -DMEAO_X_PHASE_CLOCKS=1): the workgroups with blockIdx.x % 32 == 0 stamp their phases, a white tile phase 23 instead of
phases 2..7.  384 x 384 is 36 tiles of 64 x 64: workgroups 0 (tile 0, a border tile: never white) and 32 (tile 4 = (4, 0), a
from-raw tile) are sampled.  A constant frame must stamp phase 23 from the four waves of tile 4 and phase 2 (H-blur) from those of
tile 0 only; an S2 frame, in which the oracle finds tile 4's window not white, must stamp no phase 23 at all.  Run by
tests/test_white_tiles_gpu.py::test_the_white_path_runs.

The same for the input classes of test_white_tiles_gpu.py: tile 4 stamps phase 23 from all four waves exactly when the oracle finds
its window white and no hi-res texel of it is NaN -- all-sky frames under both Z conventions, the constant plane as UNORM16 depth,
the constant plane just inside each edge of the exact-division range (the values helpers.exact_range_edges bisects), and NOT with a
NaN on an odd texel of tile 4 (white window, unclean lane) nor on the radial gradient, whose white tiles at this size are the four
centre ones (the sampled workgroups are fixed: ids 0 and 32 = tiles 0 and 4 under xcd_contiguous).  A white tile WITH a depth
gradient: the radial gradient of a 768 x 768 frame cropped so that its centre lies at (192, 0), with two levels -- the oracle finds
tile 4 white there, over 2 820 distinct depth values -- must stamp phase 23 too ("radial_top").
Outcome on an MI355X: every class the oracle finds white and clean stamped phase 23 from four waves; no missed fast path."""
import ctypes as C, dataclasses, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from miniengineao_amd import _lib as L, synth
from oracle import oracle as O
from tests import helpers as H
from tests import white_tiles as WT

O.build()
w = h = 384
s = H.settings(O, w, h)
read = L.load().meao_x_phase_clocks
read.restype, read.argtypes = C.c_int, [C.POINTER(C.c_uint64 * 64)]
buf = (C.c_uint64 * 64)()
bad = 0
conv = dataclasses.replace(synth.DEFAULT_CAMERA, reversed_z=False)
nan_frame = WT.flat_frame(w, h)
nan_frame[33, 256 + 37] = np.nan                 # odd row, odd column of tile 4: wave 0 of pass 1; no level is made of it
# (name, the oracle's input, Settings, the library's depth_format, a NaN in tile 4)
classes = [("flat", WT.flat_frame(w, h), s, L.DEPTH_F32, False), ("S2", synth.make("S2", w, h, seed=7), s, L.DEPTH_F32, False),
           ("sky", WT.sky_frame(True, w, h), s, L.DEPTH_F32, False),
           ("sky_convz", WT.sky_frame(False, w, h), H.settings(O, w, h, cam=conv), L.DEPTH_F32, False),
           ("flat_unorm16", O.encode_depth(WT.flat_frame(w, h), O.DEPTH_UNORM16), H.settings(O, w, h, depth_format=O.DEPTH_UNORM16),
            L.DEPTH_UNORM16, False),
           ("radial", synth.radial_gradient(w, h), s, L.DEPTH_F32, False), ("nan_odd", nan_frame, s, L.DEPTH_F32, True)]
radial_top = np.ascontiguousarray(synth.radial_gradient(768, 768)[384:768, 192:576])
assert len(np.unique(radial_top[0:64, 256:320])) > 1000
classes.append(("radial_top", radial_top, H.settings(O, w, h, num_levels=2), L.DEPTH_F32, False))
for edge, (field, inside, _) in sorted(H.exact_range_edges(L.load()).items()):
    classes.append(("inside_" + edge, WT.flat_frame(w, h), H.settings(O, w, h, **{field: inside}), L.DEPTH_F32, False))
expected = {"flat": True, "S2": False, "sky": True, "sky_convz": True, "flat_unorm16": True, "radial": False, "radial_top": True, "nan_odd": False,
            "inside_upsample_low": True, "inside_upsample_high": True, "inside_noise_high": True}
for name, depth, sc, fmt, unclean in classes:
    want = O.run(depth, sc)
    window_white = WT.window_white(WT.low_ao(want, sc), 4, 0)
    white = window_white and not unclean
    assert white == expected[name], (name, window_white)         # what the oracle says of the class is what this check was written for
    assert window_white or not unclean
    ao = H.component(sc, debug={L.DEBUG_FINAL_SMALL_MAX_TILES: 0}, depth_format=fmt)
    assert read(C.byref(buf)) == 0            # clear
    got = ao.render(depth)
    assert read(C.byref(buf)) == 0
    hostile = ao.hostile_frames()
    ao.close()
    white_waves, hblur_waves, fill_waves = int(buf[32 + 23]), int(buf[32 + 2]), int(buf[32 + 0])
    print(name, "waves: fill", fill_waves, "H-blur", hblur_waves, "white path", white_waves)
    ok = np.array_equal(got, want["result"]) and fill_waves == 8 and hostile == 0
    ok = ok and ((white_waves, hblur_waves) == (4, 4) if white else (white_waves, hblur_waves) == (0, 8))
    if not ok:
        bad += 1
        print("MISMATCH", name)
sys.exit(1 if bad else 0)
