"""Frames 1-3 of tests/test_white_tiles_gpu.py, and the side and NaN frames of tests/test_white_tiles_window_gpu.py, through ONE
build of libmeao_hip.so (MEAO_LIB_PATH selects it), plain (64 x 64 and 64 x 32 tiles) and as pipelined batches through the fused last kernel, the whole result against the oracle.  Run by
tests/test_white_tiles_gpu.py::test_variant_libraries, one child per variant library."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from miniengineao_amd import _lib as L
from oracle import oracle as O
from tests import helpers as H
from tests import white_tiles as WT

O.build()
dev = torch.device("cuda", 0)
s = H.settings(O, WT.W, WT.H)
frames = {"flat": WT.flat_frame(), "apron": WT.apron_frame(), "nan_odd": WT.texel_frame(WT.ODD_TEXEL, np.float32(np.nan))}
# the four side frames of the window plan (darkness only in the two outermost lines of one side of tile (2, 2)) and two frames of
# NaNs at every lane position (tests/test_white_tiles_window_gpu.py), for both tile heights
for tile_h in (64, 32):
    for i, spot in enumerate(WT.window_plan(tile_h)["sides"][:4]):
        frames["side%d_%d" % (i, tile_h)] = WT.block_frame(*spot["at"])
    for i, (d, _) in enumerate(WT.nan_frames(tile_h)[:2]):
        frames["nans%d_%d" % (i, tile_h)] = d
want = {k: O.run(d, s, result_only=True)["result"] for k, d in frames.items()}
bad = 0
for debug in ({L.DEBUG_FINAL_SMALL_MAX_TILES: 0}, None):
    ao = H.component(s, debug=debug)
    for k, d in frames.items():
        if not np.array_equal(ao.render(d), want[k]):
            bad += 1
            print("MISMATCH plain", k, debug)
    ao.close()
seq = [["flat", "apron"], ["apron", "nan_odd"], ["nan_odd", "flat"], ["side1_64", "nans0_64"], ["side3_64", "flat"]]
dd = [[torch.from_numpy(frames[n]).to(dev) for n in b] for b in seq]
out = [[torch.zeros((WT.H, WT.W), dtype=torch.uint8, device=dev) for _ in b] for b in seq]
ao = H.component(s, max_batch=2, pipelined=True)
st = torch.cuda.current_stream(dev).cuda_stream
for k in range(len(seq)):
    if k + 1 < len(seq):
        ao.prefetch_device([t.data_ptr() for t in dd[k + 1]])
    ao.execute_device([t.data_ptr() for t in dd[k]], [t.data_ptr() for t in out[k]], st)
torch.cuda.synchronize(dev)
for k, b in enumerate(seq):
    for f, n in enumerate(b):
        if not np.array_equal(out[k][f].cpu().numpy(), want[n]):
            bad += 1
            print("MISMATCH pipelined", k, f, n)
ao.close()
print("white tiles through", os.environ.get("MEAO_LIB_PATH", "product"), "ok" if bad == 0 else f"{bad} mismatches")
sys.exit(1 if bad else 0)
