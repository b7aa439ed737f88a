"""Mixed-size batches on the GPU (meao_execute_batch_extents): one size per frame inside the context's capacity.

A context of 400 x 272, max_batch 8.  The result and every valid debug buffer of EVERY frame of a mixed call are compared, NaN-aware,
with the CPU oracle run at that frame's own size and parameters (oracle.run with the frame's Settings), and every output surface
lies inside a sentinel-filled allocation whose other bytes must come back untouched.  A frame's contents depend on its size and
a seed only, so the orderings and the launch-structure variants share one oracle run per frame.

Sizes: (33, 17) has one tile in every pass of every tiling; 400 x 272 is the capacity; the "tile edge" list sits on and one past
the 64 / 128 / 256 texel tile widths and the 32 / 64 row tile heights of the passes."""
import dataclasses

import numpy as np
import pytest

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import helpers as H

pytestmark = pytest.mark.gpu

CTX = (400, 272)
MAX_BATCH = 8
ORDER = [(33, 17), (400, 272), (200, 120), (97, 61)]
ORDERINGS = {"small_first": ORDER, "reversed": ORDER[::-1], "largest_last": [(33, 17), (200, 120), (97, 61), (400, 272)]}
EDGES = [(64, 64), (65, 33), (128, 32), (129, 65), (256, 64), (257, 31)]
ALIGNED = [(64, 64), (128, 32), (256, 64), (400, 272)]        # every width % 8 == 0
SENTINEL = 0xA5
GUARD = 256                                                    # bytes in front of and behind every output surface
BIG = 1 << 20
PASS_DOWNSAMPLE = 0
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

_frames, _wants, _lin = {}, {}, []


def base_settings(oracle, **kw):
    """The oracle Settings of the 400 x 272 context (proj00 of that aspect)."""
    return H.settings(oracle, *CTX, cam=CAM, **kw)


def frame_settings(base, w, h, f=None, own_camera=False):
    """Frame f's Settings at its own size: the context's parameters, or (f given) parameters of its own."""
    s = dataclasses.replace(base, width=w, height=h)
    if f is not None:
        s = dataclasses.replace(s, intensity=1.0 + 0.25 * f, thickness_modifier=1.0 + 0.5 * f, proj00=CAM.proj00(w, h))
    return s


def params_of(s):
    return FrameParams(intensity=s.intensity, thicknessModifier=s.thickness_modifier, projection00=s.proj00)


def linearize():
    if not _lin:
        import tempfile
        from tests.test_linear_depth_gpu import build_linearize
        _lin.append(build_linearize(tempfile.mkdtemp()))
    return _lin[0]


def frame(oracle, w, h, fmt=F32, hostile=False, seed=0):
    """-> (the oracle's input frame, the library's input frame); one frame per size, format and seed."""
    key = (w, h, fmt, hostile, seed)
    if key not in _frames:
        raw = H.hostile_frame(w, h, 7 + seed, cam=CAM) if hostile else synth.occluder_field(w, h, seed=w * 1000 + h + seed, cam=CAM)
        if fmt == U16:
            enc = oracle.encode_depth(raw, U16)
            _frames[key] = (enc, enc)
        elif fmt == LF32:
            from tests.test_linear_depth_gpu import to_linear
            _frames[key] = to_linear(linearize(), raw, CAM)
        else:
            _frames[key] = (raw, raw)
    return _frames[key]


def want_of(oracle, key, depth, s):
    k = (key, dataclasses.astuple(s))
    if k not in _wants:
        _wants[k] = oracle.run(depth, s, nthreads=8)
    return _wants[k]


def ao_dtype(s):
    return np.uint8 if s.ao_format == L.AO_R8 else np.uint16


class Surface:
    """One frame's device surface of `pitch` texels per row inside an allocation with GUARD bytes of SENTINEL on both sides; the
    row padding holds SENTINEL bytes too.  intact(): every byte outside the w x h texels is still what was uploaded."""

    def __init__(self, torch, w, h, dtype, pitch, content=None):
        self.w, self.h, self.dtype, self.pitch = w, h, np.dtype(dtype), pitch
        body = np.full(h * pitch * self.dtype.itemsize, SENTINEL, np.uint8).view(self.dtype).reshape(h, pitch)
        if content is not None:
            body[:, :w] = content
        guard = np.full(GUARD, SENTINEL, np.uint8)
        self.host = np.concatenate([guard, body.view(np.uint8).ravel(), guard])
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    @property
    def ptr(self):
        return self.dev.data_ptr() + GUARD

    @property
    def pitch_bytes(self):
        return 0 if self.pitch == self.w else self.pitch * self.dtype.itemsize

    def read(self):
        got = self.dev.cpu().numpy()
        body = got[GUARD:len(got) - GUARD].view(self.dtype).reshape(self.h, self.pitch)
        texels = body[:, :self.w].copy()
        rest = got.copy()
        rest[GUARD:len(got) - GUARD].view(self.dtype).reshape(self.h, self.pitch)[:, :self.w] = \
            self.host[GUARD:len(got) - GUARD].view(self.dtype).reshape(self.h, self.pitch)[:, :self.w]
        return texels, np.array_equal(rest, self.host)


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
            self.depth.append(Surface(torch, w, h, lib_in.dtype, dpitch, lib_in))
            self.out.append(Surface(torch, w, h, ao_dtype(s), opitch))
        self.params = [params_of(s) for s in self.settings] if per_frame else None
        self.extents = [(w, h, d.pitch_bytes, o.pitch_bytes) for (w, h), d, o in zip(self.sizes, self.depth, self.out)]

    def execute(self, ao):
        ao.execute_device([d.ptr for d in self.depth], [o.ptr for o in self.out], params=self.params, extents=self.extents)

    def want(self, f):
        return want_of(self.oracle, self.keys[f], self.oracle_in[f], self.settings[f])

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


# ---- orderings, tile edges, capacity

@pytest.mark.parametrize("order", sorted(ORDERINGS))
@pytest.mark.parametrize("per_frame", [False, True])
def test_orderings(oracle, order, per_frame):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        call = MixedCall(torch, oracle, base, ORDERINGS[order], per_frame=per_frame)
        call.execute(ao)
        call.check(ao, what=order)
        # the view of a buffer has the frame's own size too
        f = ORDERINGS[order].index((97, 61))
        view = ao.debug_view(10, frame=f)
        assert view.shape == (61, 97) and np.array_equal(view, oracle.debug_view(call.want(f), 10, call.settings[f]))
    finally:
        ao.close()


def test_tile_edges(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        call = MixedCall(torch, oracle, base, EDGES, per_frame=True)
        call.execute(ao)
        call.check(ao, what="edges")
    finally:
        ao.close()


def test_capacity_is_the_reservation(oracle):
    """The same sizes inside meao_reserve(400, 272) on a context currently resized to 200 x 120: the capacity bounds them, the
    context's size is neither read nor changed."""
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        ao.reserve(*CTX)
        ao.resize(200, 120)
        for sizes in (ORDER, EDGES):
            call = MixedCall(torch, oracle, base, sizes)
            call.execute(ao)
            call.check(ao, what="reserved")
        assert (ao.width, ao.height) == (200, 120) and ao.capacity == CTX
        # a uniform call at the context's own size afterwards
        after = MixedCall(torch, oracle, base, [(200, 120)] * 2)
        ao.execute_device([d.ptr for d in after.depth], [o.ptr for o in after.out])
        after.check(ao, debug_buffers=False, what="uniform at 200 x 120")
    finally:
        ao.close()


# ---- every guarded kernel, under mixed sizes

@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_launch_structures_and_configurations(oracle, name):
    import torch
    run_variant(torch, oracle, name)


@pytest.mark.parametrize("column", sorted(set(COLUMNS) - {"r8_rtz_exact"}))
def test_other_columns(oracle, column):
    import torch
    run_variant(torch, oracle, "defaults", column=column)


TRACE_CHILD = r"""
import sys
import torch
from oracle import oracle as O
from tests import test_mixed_size_gpu as M
O.build()
for name in sorted(M.VARIANTS):
    M.run_variant(torch, O, name, debug_buffers=False)
print("mixed-size trace child ok")
"""


def test_every_per_frame_kernel_family_runs_in_a_mixed_call(tmp_path):
    """The child makes mixed calls only (R8 / RTZ / exact column): every *_frames family except the fused last kernel must show
    in its trace, each variant's own kernels by name, and no kernel of the shared calls."""
    k = H.kernel_trace(tmp_path, TRACE_CHILD)
    assert "mixed-size trace child ok" in k.stdout
    for family in FAMILIES:
        assert k[family] > 0, (family, k.short)
    assert k[FUSED] == 0 and k["upsample_final_with_next_downsample_kernel"] == 0
    for shared in ("downsample_kernel", "render_kernel", "render_small_kernel", "upsample_kernel", "upsample_final_kernel",
                   "upsample_final_small_kernel", "upsample_three_level_kernel", "upsample_two_level_kernel"):
        assert k[shared] == 0, (shared, k.short)
    from tests import kernel_inventory as K
    cols = {K.column_of(n) for n in k.short if K.column_of(n) and K.column_of(n)[0] != "ds"}
    assert cols == {("0", "false", "0")}, cols


# ---- the call's launch shape

def l1_tiles(sizes):
    """64 x 32 tiles of the L2 -> L1 pass, summed over the frames."""
    half = lambda v: (v + 1) // 2
    return sum(((half(w) + 63) // 64) * ((half(h) + 31) // 32) for w, h in sizes)


THRESHOLD_CHILD = r"""
import sys
import torch
from oracle import oracle as O
from miniengineao_amd import _lib as L
from tests import test_mixed_size_gpu as M
O.build()
base = M.base_settings(O)
for limit in (int(sys.argv[1]), int(sys.argv[1]) - 1):
    ao = M.context(base, debug={L.DEBUG_NESTED_MAX_TILES: limit})
    call = M.MixedCall(torch, O, base, M.ORDER)
    call.execute(ao)
    call.check(ao, debug_buffers=False)
    ao.close()
print("threshold child ok")
"""


def test_thresholds_compare_the_sum_over_the_frames(tmp_path):
    total = l1_tiles(ORDER)
    assert total == 1 + 4 * 5 + 2 * 2 + 1 * 1 and total != len(ORDER) * l1_tiles(ORDER[:1]) and total != len(ORDER) * l1_tiles([CTX])
    k = H.kernel_trace(tmp_path, THRESHOLD_CHILD, [str(total)])
    assert "threshold child ok" in k.stdout
    # NESTED_MAX_TILES = the sum: the three-level launch; one less: the two-level launch and L2 -> L1 on its own
    assert k["upsample_three_level_frames_kernel"] == 1 and k["upsample_two_level_frames_kernel"] == 1, k.short


VECTOR_CHILD = r"""
import torch
from oracle import oracle as O
from tests import test_mixed_size_gpu as M
O.build()
base = M.base_settings(O)
ao = M.context(base)
for sizes in (M.ALIGNED, M.ALIGNED[:3] + [(97, 61)]):
    call = M.MixedCall(torch, O, base, sizes)
    call.execute(ao)
    call.check(ao, debug_buffers=False)
ao.close()
print("vector child ok")
"""


def test_vector_forms_need_every_frame_eligible(tmp_path):
    from tests import kernel_inventory as K
    k = H.kernel_trace(tmp_path, VECTOR_CHILD)
    assert "vector child ok" in k.stdout
    ds = [K.split(n)[1][0] for n in k.short if K.split(n)[0] == "downsample_frames_kernel"]
    assert ds == ["true", "false"], k.short           # all widths % 8 == 0: VEC; one odd width: the scalar form for the call


# ---- state

def uniform_batch(torch, oracle, base, n, seed):
    return MixedCall(torch, oracle, base, [CTX] * n, seed=seed)


def execute_uniform(ao, b):
    ao.execute_device([d.ptr for d in b.depth], [o.ptr for o in b.out])


def downsample_ms(ao, b):
    """The DOWNSAMPLE slot of executing the uniform batch `b` alone: 0 = that call launched no downsample pass."""
    ao.set_profiling(True)
    execute_uniform(ao, b)
    ms, n = ao.pass_times_ms()
    assert n == 1
    return ms[PASS_DOWNSAMPLE]


def colour(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 0x7C00, (h, w, 4)) | (rng.integers(0, 2, (h, w, 4)) << 15)).astype(np.uint16)


def test_uniform_call_after_a_mixed_call(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        MixedCall(torch, oracle, base, ORDER).execute(ao)
        b = uniform_batch(torch, oracle, base, 3, seed=1)
        execute_uniform(ao, b)
        b.check(ao, what="uniform after mixed")      # (debug buffers at the context's size again)
        # the delegating form: every extent the context's size, one pair of pitches
        c = uniform_batch(torch, oracle, base, 2, seed=2)
        c.execute(ao)
        c.check(ao, what="uniform through the extents call")
    finally:
        ao.close()


def test_announcement_is_carried_as_its_own_launch(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        nxt = uniform_batch(torch, oracle, base, 2, seed=3)
        ao.prefetch_device([d.ptr for d in nxt.depth])
        call = MixedCall(torch, oracle, base, ORDER)
        call.execute(ao)
        assert downsample_ms(ao, nxt) == 0             # the mixed call carried the announced pass and promoted it
        nxt.check(ao, debug_buffers=False, what="announced batch")
        call.check(ao, debug_buffers=False, what="carrying mixed call")
        # a ready set is consumed unmatched by a mixed call: the batch it was made for runs its own pass afterwards
        again = uniform_batch(torch, oracle, base, 2, seed=4)
        ao.prefetch_device([d.ptr for d in again.depth])
        execute_uniform(ao, nxt)
        call.execute(ao)
        assert downsample_ms(ao, again) > 0
        again.check(ao, debug_buffers=False, what="after the consumed set")
    finally:
        ao.close()


def test_waiting_composite_is_flushed_first(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        b = uniform_batch(torch, oracle, base, 2, seed=5)
        execute_uniform(ao, b)
        before = [colour(*CTX, 70 + f) for f in range(2)]
        col = [torch.from_numpy(c.view(np.int16).copy()).cuda() for c in before]
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [o.ptr for o in b.out], [c.data_ptr() for c in col])
        assert ao.composite_pending
        call = MixedCall(torch, oracle, base, ORDER)
        call.execute(ao)
        assert not ao.composite_pending
        call.check(ao, debug_buffers=False, what="mixed call behind a composite")
        for f in range(2):
            want = before[f].copy()
            oracle.composite(np.ascontiguousarray(b.want(f)["result"]), want, L.COMPOSITE_MULTIPLY, L.AO_R8)
            assert np.array_equal(col[f].cpu().numpy().view(np.uint16), want), f
    finally:
        ao.close()


def test_refused_call_leaves_the_state_untouched(oracle):
    """At 400 x 272 an announced pass does not fit the last kernel's grid (36 lean tiles, 35 workgroups) and runs as a launch of its
    own, timed in the DOWNSAMPLE slot of a call that was itself prefetched -- so the ready set and the announcement are examined
    one after the other, each by a consuming call that carries nothing."""
    import torch
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        first, ready, filler, announced = (uniform_batch(torch, oracle, base, 2, seed=s) for s in (6, 7, 8, 9))
        call = MixedCall(torch, oracle, base, ORDER, per_frame=True)
        ptrs = ([d.ptr for d in call.depth], [o.ptr for o in call.out])
        bad_size = list(call.extents)
        bad_size[2] = (401, 120, 0, 0)
        bad_pitch = list(call.extents)
        bad_pitch[3] = (97, 61, 96 * 4, 0)                           # smaller than frame 3's own row of 97 texels
        bad_ao_pitch = list(call.extents)
        bad_ao_pitch[0] = (33, 17, 0, 32)                            # ... and an AO pitch smaller than frame 0's row
        bad_params = list(call.params)
        bad_params[1] = dataclasses.replace(bad_params[1], intensity=float("nan"))

        def refuse_all():
            for extents, params, match in ((bad_size, call.params, r"extents\[2\]\.width/height"),
                                           ([(0, 5, 0, 0)] + call.extents[1:], call.params, r"extents\[0\]\.width/height"),
                                           ([(40000, 5, 0, 0)] + call.extents[1:], call.params, r"extents\[0\]\.width/height"),
                                           (bad_pitch, call.params, r"extents\[3\]\.depth_pitch"),
                                           (bad_ao_pitch, call.params, r"extents\[0\]\.ao_pitch"),
                                           (call.extents, bad_params, r"params\[1\]")):
                with pytest.raises(L.MeaoError, match="meao_execute_batch_extents: " + match) as e:
                    ao.execute_device(*ptrs, params=params, extents=extents)
                assert e.value.status == L.ERR_INVALID_ARGUMENT

        # a ready set
        ao.prefetch_device([d.ptr for d in ready.depth])
        execute_uniform(ao, first)
        refuse_all()
        assert downsample_ms(ao, ready) == 0                         # it was still there: no downsample launch
        # an announcement and a waiting composite
        ao.prefetch_device([d.ptr for d in announced.depth])
        before = [colour(*CTX, 80 + f) for f in range(2)]
        col = [torch.from_numpy(c.view(np.int16).copy()).cuda() for c in before]
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [o.ptr for o in first.out], [c.data_ptr() for c in col])
        refuse_all()
        assert ao.composite_pending                                  # the composite still waits
        execute_uniform(ao, filler)                                  # carries the announced pass; the composite rides in its render kernel
        assert not ao.composite_pending
        assert downsample_ms(ao, announced) == 0                     # the announcement was still there
        ao.synchronize()
        for o in call.out:
            assert o.read()[1] and np.all(o.read()[0].view(np.uint8) == SENTINEL)      # no refused call launched anything
        for b, what in ((first, "first"), (ready, "ready"), (filler, "filler"), (announced, "announced")):
            b.check(ao, debug_buffers=False, what=what)
        for f in range(2):
            want = before[f].copy()
            oracle.composite(np.ascontiguousarray(first.want(f)["result"]), want, L.COMPOSITE_MULTIPLY, L.AO_R8)
            assert np.array_equal(col[f].cpu().numpy().view(np.uint16), want), f
        # without a reservation the capacity is the context's size
        ao.resize(200, 120)
        with pytest.raises(L.MeaoError, match=r"extents\[1\]\.width/height"):
            ao.execute_device(*ptrs, params=call.params, extents=call.extents)
    finally:
        ao.close()


# ---- the pool

@pytest.mark.parametrize("members", [2, 3])
def test_pool(oracle, members):
    import torch
    from miniengineao_amd import AmbientOcclusionPool
    base = base_settings(oracle)
    sizes = ORDER + [(129, 65)]                                        # n = 5: no multiple of 2 or 3
    pool = AmbientOcclusionPool(*CTX, [0] * members, max_batch=MAX_BATCH, near_clip=base.near_clip, far_clip=base.far_clip,
                                projection00=base.proj00, reversed_z=base.reversed_z)
    try:
        for per_frame in (False, True):
            call = MixedCall(torch, oracle, base, sizes, per_frame=per_frame)
            pool.execute_device([d.ptr for d in call.depth], [o.ptr for o in call.out], params=call.params, extents=call.extents)
            pool.synchronize()
            for f, (w, h) in enumerate(sizes):
                got, intact = call.out[f].read()
                assert np.array_equal(got, call.want(f)["result"]), (members, per_frame, f, H.diff_report("result", got, call.want(f)["result"]))
                assert intact, (members, per_frame, f)
        # n < members: the members dealt nothing sit the call out
        one = MixedCall(torch, oracle, base, [(97, 61)])
        pool.execute_device([one.depth[0].ptr], [one.out[0].ptr], extents=one.extents)
        pool.synchronize()
        assert np.array_equal(one.out[0].read()[0], one.want(0)["result"])
        # every member's share is validated before any member enqueues: frame 3 (member 3 mod G) is too large
        call = MixedCall(torch, oracle, base, sizes)
        bad = list(call.extents)
        bad[3] = (97, 273, 0, 0)
        with pytest.raises(L.MeaoError, match=r"meao_pool_execute_batch_extents: member %d .*extents\[%d\]\.width/height" % (3 % members, 3 // members)) as e:
            pool.execute_device([d.ptr for d in call.depth], [o.ptr for o in call.out], extents=bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        pool.synchronize()
        for o in call.out:
            assert np.all(o.read()[0].view(np.uint8) == SENTINEL)
    finally:
        pool.close()


def test_tensors_of_different_shapes(oracle):
    """execute_tensors with a list of 2-D tensors: crops of larger surfaces bring their own row strides as pitches."""
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        depth, keys = [], []
        for f, (w, h) in enumerate(ORDER):
            raw, _ = frame(oracle, w, h)
            if f % 2:
                surface = torch.full((h + 3, w + 5 + f), 0.25, dtype=torch.float32, device="cuda")
                surface[1:1 + h, 2:2 + w] = torch.from_numpy(raw).cuda()
                depth.append(surface[1:1 + h, 2:2 + w])
            else:
                depth.append(torch.from_numpy(raw).cuda())
        outs = ao.execute_tensors(depth)
        torch.cuda.synchronize()
        for f, (w, h) in enumerate(ORDER):
            s = frame_settings(base, w, h)
            want = want_of(oracle, (w, h, F32, False, 0), frame(oracle, w, h)[0], s)["result"]
            assert tuple(outs[f].shape) == (h, w) and np.array_equal(outs[f].cpu().numpy(), want), f
    finally:
        ao.close()


# ---- what only the testhooks variant library can show

def test_mixed_calls_neither_allocate_nor_synchronise():
    """Ten mixed DEVICE calls with every allocation set to fail: both meao_test_counters unchanged, every frame exact
    (tests/mixed_size_testhooks_check.py)."""
    H.run_against_testhooks("mixed_size_testhooks_check.py")
