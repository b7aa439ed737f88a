"""The mixed-size suite's calls (tests/test_mixed_size_gpu.py, its traced children and tests/mixed_size_testhooks_check.py): a context of
400 x 272, the size lists, the launch-structure variants, and MixedCall -- the surfaces, extents and expectations of one mixed call."""
import dataclasses

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import gpu_kit
from tests import helpers as H
from tests.helpers import params_of, want_of
from tests.linear_depth import linearize, to_linear

CTX = (400, 272)
MAX_BATCH = 8
ORDER = [(33, 17), (400, 272), (200, 120), (97, 61)]
ORDERINGS = {"small_first": ORDER, "reversed": ORDER[::-1], "largest_last": [(33, 17), (200, 120), (97, 61), (400, 272)]}
EDGES = [(64, 64), (65, 33), (128, 32), (129, 65), (256, 64), (257, 31)]
ALIGNED = [(64, 64), (128, 32), (256, 64), (400, 272)]        # every width % 8 == 0
SENTINEL = gpu_kit.SENTINEL
GUARD = 256                                                    # bytes in front of and behind every surface
BIG = 1 << 20
F32, U16, LF32 = L.DEPTH_F32, L.DEPTH_UNORM16, L.DEPTH_LINEAR_F32
CAM = synth.Camera(near=0.1, far=128.0, reversed_z=True)       # far a power of two: linear z = distance x far exactly

# (AOFMT, RTNE, DIV) columns: the settings that select each (tests/test_kernel_coverage_gpu.py)
COLUMNS = {
    "r8_rtz_exact": dict(),
    "r8_rtz_ieee": dict(upsample_tolerance=-14.0),
    "r8_rtne": dict(f16_rounding=1),
    "f16_rtz_exact": dict(ao_format=1),
    "f16_rtz_ieee": dict(ao_format=1, upsample_tolerance=-14.0),
    "f16_rtne": dict(ao_format=1, f16_rounding=1),
}

# Launch structures and configurations under mixed sizes, in the R8 / RTZ / exact column: name -> (meao_debug_set overrides,
# oracle Settings fields, depth format, pitched, hostile frame, the per-frame kernel templates the call must launch)
VARIANTS = {
    "defaults": ({}, {}, F32, False, None,
                 ["downsample_frames_kernel", "render_small_frames_kernel", "upsample_three_level_frames_kernel",
                  "upsample_final_small_frames_kernel"]),
    "nested_0": ({L.DEBUG_NESTED_MAX_TILES: 0}, {}, F32, False, None, ["upsample_two_level_frames_kernel", "upsample_frames_kernel"]),
    "nested_large": ({L.DEBUG_NESTED_MAX_TILES: BIG}, {}, F32, False, None, ["upsample_three_level_frames_kernel"]),
    "separate_blends": ({L.DEBUG_FUSE_COARSE_BLEND: 0}, {}, F32, False, None, ["upsample_frames_kernel"]),
    "no_small_tiles": ({L.DEBUG_RENDER_SMALL_MAX_TILES: 0, L.DEBUG_FINAL_SMALL_MAX_TILES: 0, L.DEBUG_DS_SMALL_MAX_TILES: 0}, {}, F32,
                       False, None, ["downsample_frames_kernel", "render_frames_kernel", "upsample_final_frames_kernel"]),
    "small_tiles": ({L.DEBUG_RENDER_SMALL_MAX_TILES: BIG, L.DEBUG_FINAL_SMALL_MAX_TILES: BIG, L.DEBUG_DS_SMALL_MAX_TILES: BIG}, {}, F32,
                    False, None, ["downsample_frames_kernel", "render_small_frames_kernel", "upsample_final_small_frames_kernel"]),
    "blend_tall": ({L.DEBUG_NESTED_MAX_TILES: 0, L.DEBUG_BLEND_TALL_MIN_TILES: 1}, {}, F32, False, None,
                   ["upsample_two_level_frames_kernel", "upsample_blend_tall_frames_kernel"]),
    "hq_levels_2": ({}, dict(hq_levels=2), F32, False, None, ["render_wide_frames_kernel"]),
    "exhaustive": ({}, dict(sample_set=L.SAMPLES_EXHAUSTIVE), F32, False, None, ["render_frames_kernel"]),
    "pitched_small": ({L.DEBUG_FINAL_SMALL_MAX_TILES: BIG, L.DEBUG_DS_SMALL_MAX_TILES: BIG}, {}, F32, True, None,
                      ["downsample_pitched_frames_kernel", "upsample_final_small_pitched_frames_kernel"]),
    "pitched_large": ({L.DEBUG_FINAL_SMALL_MAX_TILES: 0, L.DEBUG_DS_SMALL_MAX_TILES: 0}, {}, F32, True, None,
                      ["downsample_pitched_frames_kernel", "upsample_final_pitched_frames_kernel"]),
    "linear_small": ({L.DEBUG_FINAL_SMALL_MAX_TILES: BIG}, {}, LF32, False, None,
                     ["downsample_linear_frames_kernel", "upsample_final_small_linear_frames_kernel"]),
    "linear_large": ({L.DEBUG_FINAL_SMALL_MAX_TILES: 0}, {}, LF32, True, None,
                     ["downsample_linear_frames_kernel", "upsample_final_linear_frames_kernel"]),
    "unorm16": ({}, dict(depth_format=U16), U16, False, None, ["downsample_frames_kernel", "upsample_final_small_frames_kernel"]),
    "hostile_neighbour": ({}, {}, F32, False, 2, ["render_small_frames_kernel"]),
}
FAMILIES = sorted({k for v in VARIANTS.values() for k in v[5]})
FUSED = "upsample_final_with_next_downsample_frames_kernel"

_frames = {}


def base_settings(oracle, **kw):
    """The oracle Settings of the 400 x 272 context (proj00 of that aspect)."""
    return H.settings(oracle, *CTX, cam=CAM, **kw)


def frame_settings(base, w, h, f=None, own_camera=False):
    """Frame f's Settings at its own size: the context's parameters, or (f given) parameters of its own."""
    s = dataclasses.replace(base, width=w, height=h)
    if f is not None:
        s = H.frame_settings(s, FrameParams(intensity=1.0 + 0.25 * f, thicknessModifier=1.0 + 0.5 * f, projection00=CAM.proj00(w, h)))
    return s


def frame(oracle, w, h, fmt=F32, hostile=False, seed=0):
    """-> (the oracle's input frame, the library's input frame); one frame per size, format and seed."""
    key = (w, h, fmt, hostile, seed)
    if key not in _frames:
        raw = H.hostile_frame(w, h, 7 + seed, cam=CAM) if hostile else synth.occluder_field(w, h, seed=w * 1000 + h + seed, cam=CAM)
        if fmt == U16:
            enc = oracle.encode_depth(raw, U16)
            _frames[key] = (enc, enc)
        elif fmt == LF32:
            _frames[key] = to_linear(linearize(), raw, CAM)
        else:
            _frames[key] = (raw, raw)
    return _frames[key]


class MixedCall:
    """The surfaces, extents and expectations of one mixed call on a context configured like `base`."""

    def __init__(self, torch, oracle, base, sizes, fmt=F32, per_frame=False, pitched=False, hostile=None, seed=0):
        self.oracle, self.base, self.sizes = oracle, base, list(sizes)
        self.settings, self.depth, self.out, self.keys, self.oracle_in = [], [], [], [], []
        for f, (w, h) in enumerate(self.sizes):
            s = frame_settings(base, w, h, f if per_frame else None)
            fseed = seed + 1000 * self.sizes[:f].count((w, h))           # frames of one size in one call differ
            want_in, lib_in = frame(oracle, w, h, fmt, hostile == f, fseed)
            # pitched: odd and even paddings, so that some frames lose the 4-texel forms and the call with them
            dpitch, opitch = (w + 3 + 4 * f, w + 8 + f) if pitched else (w, w)
            self.settings.append(s)
            self.oracle_in.append(want_in)
            self.keys.append((w, h, fmt, hostile == f, fseed))
            # every frame's surfaces in allocations of their own, GUARD bytes on both sides
            self.depth.append(gpu_kit.Surface(w, h, lib_in.dtype, pitch=dpitch, guard=GUARD, content=[lib_in]))
            self.out.append(gpu_kit.Surface(w, h, H.ao_dtype(s.ao_format), pitch=opitch, guard=GUARD))
        self.params = [params_of(s) for s in self.settings] if per_frame else None
        self.extents = [(w, h, d.pitch_bytes, o.pitch_bytes) for (w, h), d, o in zip(self.sizes, self.depth, self.out)]

    def execute(self, ao):
        ao.execute_device([d.ptr for d in self.depth], [o.ptr for o in self.out], params=self.params, extents=self.extents)

    def want(self, f):
        return want_of(self.oracle, self.keys[f], self.oracle_in[f], self.settings[f], nthreads=8)

    def check(self, ao, debug_buffers=True, what=""):
        ao.synchronize()
        for f, (w, h) in enumerate(self.sizes):
            want = self.want(f)
            got, intact = self.out[f].read()
            ok, _ = H.nan_aware_equal(got, want["result"])
            assert ok, (what, f, (w, h), H.diff_report("result", got, want["result"]))
            assert intact, (what, f, (w, h), "bytes outside the frame's texels were written")
        if debug_buffers:
            s0 = self.settings[0]
            for f, (w, h) in enumerate(self.sizes):
                want = self.want(f)
                for i in H.valid_debug_ids(s0.num_levels, s0.hq_levels):
                    got = ao.debug_buffer(i, frame=f)
                    assert got.shape == want[H.NAMES[i]].shape, (what, f, (w, h), H.NAMES[i], got.shape, want[H.NAMES[i]].shape)
                    ok, _ = H.nan_aware_equal(got, want[H.NAMES[i]])
                    assert ok, (what, f, (w, h), H.diff_report(H.NAMES[i], got, want[H.NAMES[i]]))


def context(base, fmt=F32, debug=None, **kw):
    return H.component(base, max_batch=MAX_BATCH, depth_format=fmt, debug=debug, **kw)


def run_variant(torch, oracle, name, sizes=ORDER, column="r8_rtz_exact", debug_buffers=True):
    debug, skw, fmt, pitched, hostile, _ = VARIANTS[name]
    base = base_settings(oracle, **{**COLUMNS[column], **skw})
    ao = context(base, fmt, debug)
    try:
        call = MixedCall(torch, oracle, base, sizes, fmt=fmt, per_frame=(name != "hostile_neighbour"), pitched=pitched, hostile=hostile)
        call.execute(ao)
        call.check(ao, debug_buffers, what=name)
        if hostile is not None:
            assert ao.hostile_frames() >> hostile & 1          # that frame ran the IEEE-division bodies, next to clean ones
    finally:
        ao.close()
