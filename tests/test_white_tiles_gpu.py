"""The white-tile shortcut of the full-resolution upsample (meao_dev_upsample.hpp, "white tile"; MEAO_X_WHITE_TILES) against the
oracle, bit for bit on the whole result, at 384 x 320 (6 x 5 tiles of 64 x 64; columns 1..4 are from-raw tiles), default camera, R8.

The frames (tests/white_tiles.py): 1 constant raw depth -- every tile white; 2 the same with a 6 x 6 darker block that three
tiles see ONLY in the apron of their low-res window; 2b ("leak") a nearer 8 x 8 block whose surroundings darken at the plane's own
depth, so that apron-only darkness CHANGES result texels inside the neighbouring tiles (a test of the tile's own texels instead of
its window would store 255 there: the window test is what this frame proves); 3 a NaN /
inf / -1 / 0 / 1 on an odd texel of a white tile (no level is made of it: the lane is not clean, the tile must take the normal
path and its IEEE redo -- the reference stores 0 for the NaN, 255 for the others); 4 the NaN on a level texel (IEEE instance:
shortcut compiled out).  Every path that instantiates the tile runs them: plain 64 x 64 and 64 x 32 tiles, the fused last
kernel of pipelined batches (asserted from the launch record: steps 1 and 2 launch no downsample pass), the pitched and the per-frame-parameter entry points, linear depth, fp16 AO (compiled out), a
frame whose last tile row is partial, and the variant libraries with the shortcut off / the window read from LowDepth1.  That the
white path is the one that runs on white tiles is read from the phase stamps of the `clocks` variant (test_the_white_path_runs)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import white_tiles as WT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALL = {L.DEBUG_FINAL_SMALL_MAX_TILES: 0}        # 64 x 64 tiles whatever the tile count (calls this small take 64 x 32 tiles)
APRON_MAP = ["WWWWWW", "WW.AWW", "WWAAWW", "WWWWWW", "WWWWWW"]


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (depth, oracle outputs); computed once, never modified."""
    s = H.settings(oracle, WT.W, WT.H)
    frames = {"flat": WT.flat_frame(), "apron": WT.apron_frame(), "leak": WT.leak_frame(), "nan_odd": WT.texel_frame(WT.ODD_TEXEL, np.float32(np.nan)),
              "nan_level": WT.texel_frame(WT.LEVEL_TEXEL, np.float32(np.nan))}
    frames.update({k + "_odd": WT.texel_frame(WT.ODD_TEXEL, v) for k, v in WT.ODD_VALUES.items()})
    out = {}
    for name, d in frames.items():
        d.setflags(write=False)
        out[name] = (d, oracle.run(d, s))
    return s, out


def same(got, want, what):
    assert np.array_equal(got, want), H.diff_report(what, got, want)


def test_the_oracle_sees_the_tiles_the_frames_are_built_for(cases):
    _, c = cases
    flat, apron, nan = c["flat"][1], c["apron"][1], c["nan_odd"][1]
    assert WT.tile_map(flat["combined1"], WT.W, WT.H) == ["WWWWWW"] * 5 and (flat["result"] == 255).all()
    tiles = WT.tile_map(apron["combined1"], WT.W, WT.H)
    assert tiles == APRON_MAP
    from_raw = "".join(row[1:5] for row in tiles)
    assert "A" in from_raw and "W" in from_raw and "." in from_raw
    # the leak frame: a from-raw tile whose interior window is white, whose apron is not, and whose RESULT is not all white
    leak = c["leak"][1]
    tiles = WT.tile_map(leak["combined1"], WT.W, WT.H)
    leaked = [(tx, ty) for ty, row in enumerate(tiles) for tx in range(1, 5)
              if row[tx] == "A" and (WT.result_tile(leak["result"], tx, ty) != 255).any()]
    assert leaked, tiles
    assert (nan["combined1"] == 255).all()
    bad = np.argwhere(nan["result"] != 255)
    assert bad.tolist() == [list(WT.ODD_TEXEL)] and nan["result"][WT.ODD_TEXEL] == 0
    for k in WT.ODD_VALUES:
        assert (c[k + "_odd"][1]["result"] == 255).all(), k
    assert "W" in "".join(WT.tile_map(c["nan_level"][1]["combined1"], WT.W, WT.H))


@pytest.mark.parametrize("debug", [TALL, None], ids=["tiles64x64", "tiles64x32"])
@pytest.mark.parametrize("name", ["flat", "apron", "leak", "nan_odd", "pinf_odd", "neg_odd", "zero_odd", "one_odd", "nan_level"])
def test_plain_sequence(cases, name, debug):
    s, c = cases
    depth, want = c[name]
    ao = H.component(s, debug=debug)
    try:
        same(ao.render(depth), want["result"], name)
        if name == "nan_level":
            assert ao.hostile_frames() == 1         # the IEEE instance ran
        else:
            assert ao.hostile_frames() == 0         # the exact-reciprocal instance ran: the one that has the shortcut
            same(ao.debug_buffer(14), want["combined1"], "combined1")
    finally:
        ao.close()


def test_pipelined_batches_through_the_fused_last_kernel(cases):
    """Three batches of two frames, each announced to the call before it (30 lean downsample tiles for 30 upsample tiles: the fused
    form applies); every batch mixes a white frame with frame 2 or the leak frame.  The launch record shows the fused form: only
    step 0 launches a downsample pass, the passes of batches 1 and 2 ran inside the last kernels of steps 0 and 1."""
    torch = pytest.importorskip("torch")
    s, c = cases
    seq = [["flat", "apron"], ["leak", "nan_odd"], ["pinf_odd", "apron"]]
    dev = torch.device("cuda", 0)
    dd = [[torch.from_numpy(np.array(c[n][0])).to(dev) for n in b] for b in seq]
    out = [[torch.zeros((WT.H, WT.W), dtype=torch.uint8, device=dev) for _ in b] for b in seq]
    ao = H.component(s, max_batch=2, pipelined=True)
    try:
        stream = torch.cuda.current_stream(dev).cuda_stream
        ds_ms = []
        for k in range(len(seq)):
            if k + 1 < len(seq):
                ao.prefetch_device([t.data_ptr() for t in dd[k + 1]])
            ao.set_profiling(True)                  # a profiling window per step
            ao.execute_device([t.data_ptr() for t in dd[k]], [t.data_ptr() for t in out[k]], stream)
            ms, execs = ao.pass_times_ms()
            assert execs == 1
            ds_ms.append(ms[L.PASS_NAMES.index("downsample")])
        torch.cuda.synchronize(dev)
        assert ds_ms[0] > 0 and ds_ms[1] == 0 and ds_ms[2] == 0, ds_ms
        for k, b in enumerate(seq):
            for f, n in enumerate(b):
                same(out[k][f].cpu().numpy(), c[n][1]["result"], (k, f, n))
    finally:
        ao.close()


@pytest.mark.parametrize("name", ["flat", "apron", "leak", "nan_odd"])
def test_pitched_entry_point(cases, name):
    """Rows width + 8 texels apart, depth and result (meao_execute_batch_pitched); the texels between the rows stay untouched."""
    torch = pytest.importorskip("torch")
    s, c = cases
    depth, want = c[name]
    dev = torch.device("cuda", 0)
    dsurf = torch.full((1, WT.H, WT.W + 8), 0.5, dtype=torch.float32, device=dev)
    osurf = torch.full((1, WT.H, WT.W + 8), 7, dtype=torch.uint8, device=dev)
    dsurf[0, :, :WT.W] = torch.from_numpy(np.array(depth)).to(dev)
    ao = H.component(s, debug=TALL)
    try:
        ao.execute_tensors(dsurf[:, :, :WT.W], osurf[:, :, :WT.W])
        torch.cuda.synchronize(dev)
        got = osurf.cpu().numpy()[0]
        same(got[:, :WT.W], want["result"], name)
        assert (got[:, WT.W:] == 7).all()
    finally:
        ao.close()


@pytest.mark.parametrize("name", ["flat", "apron", "leak", "nan_odd"])
def test_per_frame_parameter_entry_point(cases, name):
    s, c = cases
    depth, want = c[name]
    ao = H.component(s, debug=TALL)
    try:
        same(ao.render_batch([depth], params=[FrameParams()])[0], want["result"], name)
    finally:
        ao.close()


def test_linear_f32_depth(oracle):
    """Frame 1 as linear view-space depth (far_clip a power of two: z = Linearize(d) * far is exact)."""
    from miniengineao_amd import synth
    cam = synth.Camera(near=0.1, far=128.0, reversed_z=True)
    s = H.settings(oracle, WT.W, WT.H, cam=cam)
    z = np.full((WT.H, WT.W), WT.linear_z_of_constant(WT.FLAT, cam), np.float32)
    want = oracle.run(WT.flat_frame(), s)
    assert WT.tile_map(want["combined1"], WT.W, WT.H) == ["WWWWWW"] * 5 and (want["result"] == 255).all()
    ao = H.component(s, debug=TALL, depth_format=L.DEPTH_LINEAR_F32)
    try:
        same(ao.render(z), want["result"], "linear")
    finally:
        ao.close()


def test_fp16_ao_storage_has_no_shortcut(oracle):
    s = H.settings(oracle, WT.W, WT.H, ao_format=L.AO_F16)
    want = oracle.run(WT.flat_frame(), s)
    ao = H.component(s, debug=TALL)
    try:
        same(ao.render(WT.flat_frame()), want["result"], "fp16")
    finally:
        ao.close()


@pytest.mark.parametrize("h", [288, 312])
def test_partial_last_tile_row(oracle, h):
    """384 x 288: the last tile row is half a tile (its tiles read LowDepth1 and mask their rows); 384 x 312: white tiles above a
    partial last row."""
    s = H.settings(oracle, WT.W, h)
    want = oracle.run(WT.flat_frame(WT.W, h), s)
    if h == 312:
        assert "W" in "".join(WT.tile_map(want["combined1"], WT.W, h))
    ao = H.component(s, debug=TALL)
    try:
        same(ao.render(WT.flat_frame(WT.W, h)), want["result"], h)
    finally:
        ao.close()


def test_the_white_path_runs():
    """The `clocks` variant stamps the phases of one workgroup in 32; a white tile stamps phase 23 instead of 2..7.  Its child
    process runs a white frame and a frame without white tiles and compares the counts (tests/white_tiles_clocks_check.py)."""
    lib = os.path.join(ROOT, "miniengineao_amd", "lib", "variants", "libmeao_clocks.so")
    if not os.path.exists(lib):
        from miniengineao_amd import build
        build.build_variants(["clocks"], strict=True)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "white_tiles_clocks_check.py")], cwd=ROOT,
                          env=dict(os.environ, MEAO_LIB_PATH=lib), capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-1500:], proc.stderr[-1500:])


@pytest.mark.parametrize("variant", ["nowhite", "lowbuf"])
def test_variant_libraries(variant):
    """Frames 1-3 through the library built with MEAO_X_WHITE_TILES=0 (the form without the shortcut stays parity-tested) and
    through the one whose interior tiles fill their window from LowDepth1 (the shortcut's other fill path).  A library is loaded
    once per process: a child.  Built on the spot when missing -- never skipped."""
    lib = os.path.join(ROOT, "miniengineao_amd", "lib", "variants", f"libmeao_{variant}.so")
    if not os.path.exists(lib):
        from miniengineao_amd import build
        build.build_variants([variant], strict=True)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "white_tiles_variant_check.py")], cwd=ROOT,
                          env=dict(os.environ, MEAO_LIB_PATH=lib), capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, (proc.stdout[-1500:], proc.stderr[-1500:])
