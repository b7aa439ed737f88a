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
white path is the one that runs on white tiles is read from the phase stamps of the `clocks` variant (test_the_white_path_runs).

Second half: the input classes and entry points the shortcut meets in the field -- sky and half-sky frames under both Z conventions,
the radial gradient, UNORM16 and linear f32 / f16 depth, both sides of the edges of the exact-division range, far-outside intensity and
thickness, 1 and 2 levels, hq_levels, the exhaustive sample set, single-pass stereo, per-frame parameter batches inside the exact
column and with one frame outside it, pitched surfaces with a vector pitch and with pitch 389, 380 x 320, 400 x 330, 384 x 312 and the
shaded call.  The window, wave and lane tests are in tests/test_white_tiles_window_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import white_tiles as WT
from tests.helpers import frame_settings, same, want_of

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


# ---- input classes and entry points the shortcut meets in the field.  Every case: the whole result and the low-res AO against the
# oracle for 64 x 64 and 64 x 32 tiles; the oracle must find white tiles in the frame, so that no case passes because the shortcut
# never fires (which path DOES fire is read from the phase stamps: tests/white_tiles_clocks_check.py).

CAM128 = synth.Camera(near=0.1, far=128.0, reversed_z=True)
RAW_Z2 = np.float32(63.0 / 1279.0)       # with CAM128: 1279 d + 1 rounds to 64, dist = 1 / 64, z = 2.0 -- exact in f16
TILE_IDS = ["tiles64x64", "tiles64x32"]


def check_class(oracle, key, s, depth, debug, lib_depth=None, white=True, **kw):
    want = want_of(oracle, key, depth, s)
    tiles = WT.white_tiles_h(WT.low_ao(want, s), s.width, s.height, 64 if debug else 32)
    assert bool([t for t in tiles if 32 * t[0] >= 4 and 32 * t[0] + 35 < (s.width + 1) // 2]) == white, (key, tiles)
    ao = H.component(s, debug=debug, **kw)
    try:
        same(ao.render(depth if lib_depth is None else lib_depth), want["result"], key)
        assert ao.hostile_frames() == 0          # no frame here is hostile: the column depends on the parameters alone
        same(ao.debug_buffer(14 if s.num_levels > 1 else 10), WT.low_ao(want, s), "low-res AO")
    finally:
        ao.close()
    return want


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("name", ["sky", "sky_convz", "half_sky", "half_sky_convz", "radial"])
def test_field_frames(oracle, name, debug):
    cam, d = WT.field_frame(name)
    check_class(oracle, name, H.settings(oracle, WT.W, WT.H, cam=cam), d, debug)


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("name", ["flat", "half_sky"])
def test_unorm16_depth(oracle, name, debug):
    _, d = WT.field_frame(name)
    s = H.settings(oracle, WT.W, WT.H, depth_format=oracle.DEPTH_UNORM16)
    check_class(oracle, "u16_" + name, s, oracle.encode_depth(d, oracle.DEPTH_UNORM16), debug, depth_format=L.DEPTH_UNORM16)


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("fmt", ["f32", "f16"])
@pytest.mark.parametrize("name", ["flat", "half_sky"])
def test_linear_depth_classes(oracle, name, fmt, debug):
    """Linear view-space depth, far_clip 128: the plane at z = 2.0 (exact in f16), sky texels far or +inf, alternating."""
    s = H.settings(oracle, WT.W, WT.H, cam=CAM128)
    z_plane = WT.linear_z_of_constant(RAW_Z2, CAM128)
    assert z_plane == np.float32(2.0)
    d = np.full((WT.H, WT.W), RAW_Z2, np.float32)
    z = np.full((WT.H, WT.W), z_plane, np.float32)
    if name == "half_sky":
        d[:, :WT.W // 2] = 0.0
        sky = np.zeros(d.shape, bool)
        sky[:, :WT.W // 2] = True
        alt = (np.arange(d.size).reshape(d.shape) & 1) == 1
        z[sky & alt], z[sky & ~alt] = np.inf, np.float32(128.0)
    check_class(oracle, "lin_" + name, s, d, debug, lib_depth=z if fmt == "f32" else z.astype(np.float16),
                depth_format=L.DEPTH_LINEAR_F32 if fmt == "f32" else L.DEPTH_LINEAR_F16)


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("side", ["inside", "outside"])
def test_exact_range_edges_on_white_frames(oracle, meao_lib, side, debug):
    """Just inside each edge the context keeps the exact-reciprocal column (the shortcut's instance), just outside it runs IEEE
    division.  Here both sides must equal the oracle; helpers.in_exact_range only restates the library's rule.  WHICH column ran
    for these same frames and values is read from the kernel names in test_the_edges_select_the_column_on_white_frames, and that
    the white path runs just inside from the phase stamps (tests/white_tiles_clocks_check.py)."""
    for edge, (field, inside, outside) in sorted(H.exact_range_edges(meao_lib).items()):
        v = inside if side == "inside" else outside
        assert H.in_exact_range(meao_lib, **{field: v}) == (side == "inside")
        for name in ("flat", "half_sky", "radial"):
            cam, d = WT.field_frame(name)
            s = H.settings(oracle, WT.W, WT.H, cam=cam, **{field: v})
            check_class(oracle, (edge, side, name), s, d, debug)


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
def test_far_outside_intensity_and_thickness(oracle, meao_lib, debug):
    _, d = WT.field_frame("half_sky")
    for field in ("intensity", "thickness_modifier"):
        for v in H.FAR_OUTSIDE[field]:
            assert H.in_exact_range(meao_lib, **{field: v})              # these leave the exact range untouched
            want = want_of(oracle, (field, v), d, H.settings(oracle, WT.W, WT.H, **{field: v}))
            white = bool(WT.white_tiles_h(want["combined1"], WT.W, WT.H))
            check_class(oracle, (field, v), H.settings(oracle, WT.W, WT.H, **{field: v}), d, debug, white=white)


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("kw", [dict(num_levels=1), dict(num_levels=2), dict(hq_levels=2), dict(single_pass_stereo=True)],
                         ids=["levels1", "levels2", "hq2", "stereo"])
def test_level_counts_and_variants(oracle, kw, debug):
    _, d = WT.field_frame("half_sky")
    s = H.settings(oracle, WT.W, WT.H, **kw)
    want = want_of(oracle, str(kw), d, s)
    check_class(oracle, str(kw), s, d, debug, white=bool(WT.white_tiles_h(WT.low_ao(want, s), WT.W, WT.H)))


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
def test_exhaustive_sample_set(oracle, debug):
    _, d = WT.field_frame("half_sky")
    s = H.settings(oracle, WT.W, WT.H, sample_set=oracle.SAMPLES_EXHAUSTIVE)
    want = want_of(oracle, "exhaustive", d, s)
    check_class(oracle, "exhaustive", s, d, debug, white=bool(WT.white_tiles_h(want["combined1"], WT.W, WT.H)))


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("mixed", [False, True], ids=["exact_column", "one_frame_outside"])
def test_per_frame_parameter_batches(oracle, meao_lib, mixed, debug):
    """Default, inside-edge and other blur / intensity values per frame: the call stays in the exact column; with one outside-edge
    frame the whole call runs IEEE division and must still match."""
    edges = H.exact_range_edges(meao_lib)
    params = [FrameParams(), FrameParams(upsampleTolerance=edges["upsample_high"][1]), FrameParams(blurTolerance=-3.0, intensity=0.5),
              FrameParams(noiseFilterTolerance=edges["noise_high"][1]), FrameParams(upsampleTolerance=edges["upsample_low"][1])]
    if mixed:
        params[3] = FrameParams(upsampleTolerance=edges["upsample_high"][2])
    depths = [WT.field_frame(n)[1] for n in ("flat", "half_sky", "radial", "half_sky", "flat")]
    base = H.settings(oracle, WT.W, WT.H)
    ao = H.component(base, max_batch=len(depths), debug=debug)
    try:
        got = ao.render_batch(depths, params=params)
        white = 0
        for f, (d, p) in enumerate(zip(depths, params)):
            s = frame_settings(base, p)
            want = want_of(oracle, ("pf", mixed, f), d, s)
            white += len(WT.white_tiles_h(want["combined1"], WT.W, WT.H))
            same(got[f], want["result"], (f, p))
            same(ao.debug_buffer(14, frame=f), want["combined1"], ("combined1", f, p))
        assert white > 0
    finally:
        ao.close()


@pytest.mark.parametrize("pitch", [WT.W + 8, 389], ids=["vector_pitch", "pitch389"])
@pytest.mark.parametrize("name", ["sky", "half_sky"])
def test_pitched_surfaces_of_field_frames(oracle, name, pitch):
    """Pitch 389: rows are not 16-byte aligned (vec_ok false), the shortcut stands down and the normal path stores the same 255s."""
    torch = pytest.importorskip("torch")
    _, d = WT.field_frame(name)
    s = H.settings(oracle, WT.W, WT.H)
    want = want_of(oracle, name, d, s)
    dev = torch.device("cuda", 0)
    dsurf = torch.full((1, WT.H, pitch), 0.5, dtype=torch.float32, device=dev)
    osurf = torch.full((1, WT.H, pitch), 7, dtype=torch.uint8, device=dev)
    dsurf[0, :, :WT.W] = torch.from_numpy(np.array(d)).to(dev)
    ao = H.component(s, debug=TALL)
    try:
        ao.execute_tensors(dsurf[:, :, :WT.W], osurf[:, :, :WT.W])
        torch.cuda.synchronize(dev)
        got = osurf.cpu().numpy()[0]
        same(got[:, :WT.W], want["result"], (name, pitch))
        assert (got[:, WT.W:] == 7).all()
        same(ao.debug_buffer(14), want["combined1"], ("combined1", name, pitch))
    finally:
        ao.close()


@pytest.mark.parametrize("debug", [TALL, None], ids=TILE_IDS)
@pytest.mark.parametrize("w,h", [(380, 320), (400, 330), (384, 312)])
def test_frame_sizes_with_partial_tiles(oracle, w, h, debug):
    """380 x 320: the constant plane, white everywhere on the oracle -- but the low width is 190, no multiple of 4, so no tile is
    interior or from-raw and the shortcut never fires at this size: the normal path must store the same 255s.
    384 x 312, all sky: twelve white tiles above tile rows that are not (the low-res AO of the reference is not code 255 where a
    level's size is not whole -- for the plane and for the sky alike), and a partial last tile row with masked stores.
    400 x 330, all sky: a partial right column and bottom row; NO tile is white at this size, for the sky or the plane (same
    reason), so this case only shows that the result is the oracle's -- all 255 -- with the shortcut compiled in."""
    d = WT.flat_frame(w, h) if (w, h) == (380, 320) else WT.sky_frame(True, w, h)
    s = H.settings(oracle, w, h)
    want = want_of(oracle, (w, h), d, s)
    assert len(WT.white_tiles_h(want["combined1"], w, h)) == {(380, 320): 30, (384, 312): 12, (400, 330): 0}[(w, h)]
    assert (want["result"] == 255).all()
    ao = H.component(s, debug=debug)
    try:
        same(ao.render(d), want["result"], (w, h))
        same(ao.debug_buffer(14), want["combined1"], ("combined1", w, h))
    finally:
        ao.close()


def test_shaded_batch_on_half_sky(oracle):
    """meao_execute_batch_shaded: the AO of the white path composited by the same call, against oracle.composite of the oracle's AO."""
    torch = pytest.importorskip("torch")
    _, d = WT.field_frame("half_sky")
    s = H.settings(oracle, WT.W, WT.H)
    want = want_of(oracle, "half_sky", d, s)
    rng = np.random.default_rng(5)
    color = rng.random((WT.H, WT.W, 4), dtype=np.float32).astype(np.float16)
    expect = color.copy()
    oracle.composite(np.array(want["result"]), expect, L.COMPOSITE_MULTIPLY)
    dev = torch.device("cuda", 0)
    ct = torch.from_numpy(color.copy()).to(dev)[None]
    ao = H.component(s, debug=TALL)
    try:
        out = ao.execute_tensors(torch.from_numpy(np.array(d)).to(dev)[None], color=ct, mode=L.COMPOSITE_MULTIPLY)
        torch.cuda.synchronize(dev)
        same(out.cpu().numpy()[0], want["result"], "AO")
        same(ao.debug_buffer(14), want["combined1"], "combined1")
        got = ct.cpu().numpy()[0]
        assert np.array_equal(got.view(np.uint16), expect.view(np.uint16)), H.diff_report("colour", got.view(np.uint16), expect.view(np.uint16))
    finally:
        ao.close()


EDGE_TRACE_CHILD = r"""
import sys
import numpy as np
from oracle import oracle as O
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import white_tiles as WT

side = sys.argv[1]
O.build()
for edge, (field, inside, outside) in sorted(H.exact_range_edges(L.load()).items()):
    for name in ("flat", "half_sky", "radial"):
        cam, d = WT.field_frame(name)
        s = H.settings(O, WT.W, WT.H, cam=cam, **{field: inside if side == "inside" else outside})
        for debug in ({L.DEBUG_FINAL_SMALL_MAX_TILES: 0}, None):
            ao = H.component(s, debug=debug)
            got = ao.render(d)
            ao.close()
            assert np.array_equal(got, O.run(d, s, result_only=True)["result"]), (edge, name, debug)
print("white edges ok", side)
"""


@pytest.mark.parametrize("side,div", [("inside", "0"), ("outside", "1")])
def test_the_edges_select_the_column_on_white_frames(tmp_path, side, div):
    """The frames and values of test_exact_range_edges_on_white_frames in a child under the kernel trace: every kernel of the child
    is of the exact-reciprocal column just inside the edges and of the IEEE column just outside (tests/kernel_inventory.py
    column_of, as tests/test_param_domain_gpu.py reads it)."""
    from tests import kernel_inventory as K
    k = H.kernel_trace(tmp_path, EDGE_TRACE_CHILD, [side])
    assert "white edges ok" in k.stdout
    cols = {K.column_of(n) for n in k.short} - {None}
    assert cols, k.short[:20]
    assert {c[2] if c[0] != "ds" else c[1] for c in cols} == {div}, (side, sorted(cols))
