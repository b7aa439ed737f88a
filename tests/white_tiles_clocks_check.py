"""Which path the full-resolution tiles take, read from the phase stamps of the `clocks` variant library (MEAO_LIB_PATH; built
with -DMEAO_X_PHASE_CLOCKS=1): the workgroups with blockIdx.x % 32 == 0 stamp their phases, a white tile phase 23 instead of
phases 2..7.  384 x 384 is 36 tiles of 64 x 64: workgroups 0 (tile 0, a border tile: never white) and 32 (tile 4 = (4, 0), a
from-raw tile) are sampled.  A constant frame must stamp phase 23 from the four waves of tile 4 and phase 2 (H-blur) from those of
tile 0 only; an S2 frame, in which the oracle finds tile 4's window not white, must stamp no phase 23 at all.  Run by
tests/test_white_tiles_gpu.py::test_the_white_path_runs."""
import ctypes as C, os, sys
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
for name, depth, white in (("flat", WT.flat_frame(w, h), True), ("S2", synth.make("S2", w, h, seed=7), False)):
    want = O.run(depth, s)
    assert WT.window_white(want["combined1"], 4, 0) == white
    ao = H.component(s, debug={L.DEBUG_FINAL_SMALL_MAX_TILES: 0})
    assert read(C.byref(buf)) == 0            # clear
    got = ao.render(depth)
    assert read(C.byref(buf)) == 0
    ao.close()
    white_waves, hblur_waves, fill_waves = int(buf[32 + 23]), int(buf[32 + 2]), int(buf[32 + 0])
    print(name, "waves: fill", fill_waves, "H-blur", hblur_waves, "white path", white_waves)
    ok = np.array_equal(got, want["result"]) and fill_waves == 8
    ok = ok and ((white_waves, hblur_waves) == (4, 4) if white else (white_waves, hblur_waves) == (0, 8))
    if not ok:
        bad += 1
        print("MISMATCH", name)
sys.exit(1 if bad else 0)
