"""Per-frame camera and AO parameters (meao_execute_batch_params and its prefetch / pool forms) on the GPU.

Frame f of a per-frame call must equal the CPU oracle run on that frame with THAT frame's parameters -- result and
intermediates, in every launch structure the library has, plain and pipelined.
"""
import ctypes as C
import dataclasses
import zlib

import numpy as np
import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from miniengineao_amd import synth
from tests import helpers as H
from tests.helpers import encode_depth, f32, frame_settings, random_params

pytestmark = pytest.mark.gpu

PASS_DOWNSAMPLE, PASS_UPSAMPLE_3, PASS_UPSAMPLE_2 = 0, 2, 3      # meao_pass launch slots

def frame_depth(s, seed):
    """An S2 frame seen by the frame's own camera (its near / far / reversed_z)."""
    cam = synth.Camera(near=s.near_clip, far=s.far_clip, reversed_z=bool(s.reversed_z))
    d = synth.occluder_field(s.width, s.height, seed, cam=cam)
    if s.depth_format == L.DEPTH_F32:
        return d
    return encode_depth(d, s.depth_format)


def assert_frame(ao, oracle, depth, s, f, got=None, ids=None):
    want = oracle.run(depth, s, result_only=ids is None and got is not None)
    if got is not None:
        ok, _ = H.nan_aware_equal(got, want["result"])
        assert ok, (f, H.diff_report("result", got, want["result"]))
    for i in ids or ():
        g = ao.debug_buffer(i, frame=f)
        ok, _ = H.nan_aware_equal(g, want[H.NAMES[i]])
        assert ok, (f, i, H.diff_report(H.NAMES[i], g, want[H.NAMES[i]]))


def run_host(oracle, base, params, seeds, max_batch=None, debug=None, ids=None, **kw):
    n = len(params)
    sets = [frame_settings(base, p) for p in params]
    depths = [frame_depth(s, seed) for s, seed in zip(sets, seeds)]
    ao = H.component(base, max_batch=max_batch or n, debug=debug, depth_format=base.depth_format, **kw)
    try:
        outs = ao.render_batch(depths, params=params)
        for f in range(n):
            assert_frame(ao, oracle, depths[f], sets[f], f, got=outs[f], ids=ids)
    finally:
        ao.close()


def test_mixed_cameras_every_buffer(oracle):
    w, h, n = 644, 364, 8
    base = H.settings(oracle, w, h)
    params = random_params(np.random.default_rng(20261015), w, h, n)
    # the instance's own parameters are neither read nor changed: give it something no frame uses
    sets = [frame_settings(base, p) for p in params]
    depths = [frame_depth(s, 100 + f) for f, s in enumerate(sets)]
    ao = H.component(base, max_batch=n)
    try:
        ao.intensity = 3.5
        before = L.Params()
        outs = ao.render_batch(depths, params=params)
        L.check(ao._lib.meao_get_params(ao._ctx, C.byref(before)), ao._ctx)
        assert np.float32(before.intensity) == np.float32(3.5)
        for f in range(n):
            assert_frame(ao, oracle, depths[f], sets[f], f, got=outs[f], ids=H.valid_debug_ids(4))
    finally:
        ao.close()


CONFIGS = {
    "r8_rtz": dict(), "r8_rtne": dict(f16_rounding=L.F16_RTNE), "f16_rtz": dict(ao_format=L.AO_F16),
    "f16_rtne": dict(ao_format=L.AO_F16, f16_rounding=L.F16_RTNE),
    "unorm16": dict(depth_format=L.DEPTH_UNORM16), "unorm24": dict(depth_format=L.DEPTH_UNORM24),
    "depth_f16": dict(depth_format=L.DEPTH_F16),
    "levels1": dict(num_levels=1), "levels2": dict(num_levels=2), "levels3": dict(num_levels=3),
    "hq2": dict(hq_levels=2), "hq4_exhaustive": dict(hq_levels=4, sample_set=L.SAMPLES_EXHAUSTIVE),
    "exhaustive": dict(sample_set=L.SAMPLES_EXHAUSTIVE),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_configurations(oracle, name):
    w, h, n = 200, 120, 3
    base = dataclasses.replace(H.settings(oracle, w, h), **CONFIGS[name])
    params = random_params(np.random.default_rng(zlib.crc32(name.encode())), w, h, n)
    params[1] = dataclasses.replace(params[1], singlePassStereoEnabled=not params[0].singlePassStereoEnabled)
    run_host(oracle, base, params, [7 + f for f in range(n)], ids=[17, 2, 10])


# launch structures: (frames, max_batch, debug overrides, passes that must NOT have run as launches of their own)
STRUCTURES = {
    "one_frame_three_level": (1, 1, {}, [PASS_UPSAMPLE_3, PASS_UPSAMPLE_2]),
    "two_frames_three_level": (2, 2, {}, [PASS_UPSAMPLE_3, PASS_UPSAMPLE_2]),
    "two_level_and_tall_blend": (6, 6, {L.DEBUG_NESTED_MAX_TILES: 0, L.DEBUG_BLEND_TALL_MIN_TILES: 1}, [PASS_UPSAMPLE_3]),
    "no_fusion_small_tiles_off": (3, 4, {L.DEBUG_FUSE_COARSE_BLEND: 0, L.DEBUG_RENDER_SMALL_MAX_TILES: 0,
                                         L.DEBUG_FINAL_SMALL_MAX_TILES: 0, L.DEBUG_DS_SMALL_MAX_TILES: 0}, []),
    "max_batch_64": (64, 64, {}, [PASS_UPSAMPLE_3]),
}


@pytest.mark.parametrize("name", sorted(STRUCTURES))
def test_launch_structures(oracle, name):
    n, mb, debug, absent = STRUCTURES[name]
    w, h = (1920, 1080) if n <= 2 else (256, 160)
    base = H.settings(oracle, w, h)
    params = random_params(np.random.default_rng(n * 7 + mb), w, h, n)
    sets = [frame_settings(base, p) for p in params]
    depths = [frame_depth(s, 900 + f % 8) for f, s in enumerate(sets)]
    ao = H.component(base, max_batch=mb, debug=debug)
    try:
        ao.set_profiling(True)
        outs = ao.render_batch(depths, params=params)
        ms, execs = ao.pass_times_ms()
        assert execs == 1
        for p in absent:
            assert ms[p] == 0, (name, p, ms)
        for f in range(n):
            assert_frame(ao, oracle, depths[f], sets[f], f, got=outs[f])
    finally:
        ao.close()


def test_equal_params_equal_shared_call_1080p(oracle):
    import torch
    w, h, n = 1920, 1080, 4
    base = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    depths = [torch.from_numpy(synth.make("S2", w, h, seed=50 + f)).to(dev) for f in range(n)]
    a = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(n)]
    b = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(n)]
    ao = H.component(base, max_batch=n)
    try:
        ptrs = [t.data_ptr() for t in depths]
        ao.execute_device(ptrs, [t.data_ptr() for t in a])
        ao.execute_device(ptrs, [t.data_ptr() for t in b], params=[FrameParams()] * n)   # every field = the instance's
        ao.synchronize()
        for f in range(n):
            assert torch.equal(a[f], b[f]), f
    finally:
        ao.close()


@pytest.mark.parametrize("own_launch", [0, 1])
def test_pipelined_stream_changing_cameras(oracle, own_launch):
    import torch
    w, h, B, steps = 384, 256, 4, 3
    base = H.settings(oracle, w, h)
    rng = np.random.default_rng(77)
    params = [random_params(rng, w, h, B) for _ in range(steps)]
    sets = [[frame_settings(base, p) for p in ps] for ps in params]
    depths = [[frame_depth(s, 300 + 10 * k + f) for f, s in enumerate(ss)] for k, ss in enumerate(sets)]
    depths[1][1] = H.hostile_frame(w, h, 5, kinds=["nan", "neg", "huge"], density=0.002)     # odd texels only
    depths[1][1][0::2, 0::2] = frame_depth(sets[1][1], 5)[0::2, 0::2]
    depths[2][2] = H.hostile_frame(w, h, 6, density=0.01)                                     # level texels too
    # batch 2 is announced with near / far of its own and consumed with different ones: its downsample must re-run
    announced2 = [dataclasses.replace(p, nearClipPlane=f32(p.nearClipPlane * 2)) for p in params[2]]
    dev = torch.device("cuda", 0)
    dd = [[torch.from_numpy(d).to(dev) for d in ds] for ds in depths]
    out = [[torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(B)] for _ in range(steps)]
    st = torch.cuda.current_stream(dev).cuda_stream
    ao = H.component(base, max_batch=B, pipelined=True, debug={L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: own_launch})
    try:
        ds_ms = []                                  # the DOWNSAMPLE launch slot of each step, a profiling window per step
        for k in range(steps):
            if k + 1 < steps:
                ao.prefetch_device([t.data_ptr() for t in dd[k + 1]], params=announced2 if k + 1 == 2 else params[k + 1])
            ao.set_profiling(True)
            ao.execute_device([t.data_ptr() for t in dd[k]], [t.data_ptr() for t in out[k]], st, params=params[k])
            ms, execs = ao.pass_times_ms()
            assert execs == 1
            ds_ms.append(ms[PASS_DOWNSAMPLE])
        torch.cuda.synchronize(dev)
        assert ds_ms[0] > 0                         # step 0: its own pass
        if own_launch:
            assert ds_ms[1] > 0                     # step 1 reused batch 1's pass; the slot times batch 2's pass behind its last kernel
        else:
            assert ds_ms[1] == 0                    # step 1 reused batch 1's pass (carried in step 0's last kernel)
        assert ds_ms[2] > 0                         # step 2: announced with another near plane -> its pass re-ran
        for k in range(steps):
            for f in range(B):
                got = out[k][f].cpu().numpy()
                want = oracle.run(depths[k][f], sets[k][f], result_only=True)["result"]
                assert np.array_equal(got, want), (k, f, H.diff_report("result", got, want))
        lin = ao.debug_buffer(2, frame=B - 1)          # LowDepth1 of the last step: from ITS parameters
        assert H.nan_aware_equal(lin, oracle.run(depths[2][B - 1], sets[2][B - 1])["low_depth1"])[0]
    finally:
        ao.close()


def test_pool_deals_params_with_frames(oracle):
    from miniengineao_amd import AmbientOcclusionPool
    w, h, n = 256, 144, 5
    base = H.settings(oracle, w, h)
    params = random_params(np.random.default_rng(9), w, h, n)
    sets = [frame_settings(base, p) for p in params]
    depths = [frame_depth(s, 40 + f) for f, s in enumerate(sets)]
    pool = AmbientOcclusionPool(w, h, [0, 0], max_batch=3, near_clip=base.near_clip, far_clip=base.far_clip,
                                projection00=base.proj00, reversed_z=base.reversed_z)
    try:
        outs = pool.render_batch(depths, params=params)
        for f in range(n):
            want = oracle.run(depths[f], sets[f], result_only=True)["result"]
            assert np.array_equal(outs[f], want), (f, H.diff_report("result", outs[f], want))
    finally:
        pool.close()


def test_pending_composite_applied_before_per_frame_call(oracle):
    import torch
    w, h, n = 256, 160, 2
    base = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    params = random_params(np.random.default_rng(3), w, h, n)
    sets = [frame_settings(base, p) for p in params]
    depths = [frame_depth(s, 60 + f) for f, s in enumerate(sets)]
    dd = [torch.from_numpy(d).to(dev) for d in depths]
    out = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(n)]
    out2 = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(n)]
    rng = np.random.default_rng(4)
    colors = [rng.uniform(0, 2, (h, w, 4)).astype(np.float16) for _ in range(n)]
    col = [torch.from_numpy(c.view(np.int16)).to(dev) for c in colors]
    ao = H.component(base, max_batch=n)
    try:
        ao.execute_device([t.data_ptr() for t in dd], [t.data_ptr() for t in out], params=params)
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [t.data_ptr() for t in out], [t.data_ptr() for t in col])
        ao.execute_device([t.data_ptr() for t in dd], [t.data_ptr() for t in out2], params=params[::-1])
        assert not ao.composite_pending
        ao.synchronize()
        for f in range(n):
            ao_want = oracle.run(depths[f], sets[f], result_only=True)["result"]
            assert np.array_equal(out[f].cpu().numpy(), ao_want), f
            a = (ao_want.astype(np.float32) / np.float32(255)).astype(np.float32)
            want = (colors[f].astype(np.float32) * a[:, :, None]).astype(np.float16)
            got = col[f].cpu().numpy().view(np.float16)
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), f
            ao_rev = oracle.run(depths[f], sets[n - 1 - f], result_only=True)["result"]
            assert np.array_equal(out2[f].cpu().numpy(), ao_rev), f
    finally:
        ao.close()


def test_invalid_params_launch_nothing(oracle):
    import torch
    w, h, n = 256, 160, 3
    base = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    depths = [synth.make("S2", w, h, seed=70 + f) for f in range(n)]
    dd = [torch.from_numpy(d).to(dev) for d in depths]
    out = [torch.full((h, w), 0xA5, dtype=torch.uint8, device=dev) for _ in range(n)]
    params = random_params(np.random.default_rng(5), w, h, n)
    bad = list(params)
    bad[1] = dataclasses.replace(bad[1], farClipPlane=float("nan"))
    ao = H.component(base, max_batch=n)
    try:
        ao.execute_device([t.data_ptr() for t in dd], [t.data_ptr() for t in out])     # the instance's parameters applied
        ao.synchronize()
        for t in out:
            t.fill_(0xA5)
        before = L.Params()
        L.check(ao._lib.meao_get_params(ao._ctx, C.byref(before)), ao._ctx)
        with pytest.raises(L.MeaoError) as e:
            ao.execute_device([t.data_ptr() for t in dd], [t.data_ptr() for t in out], params=bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT and "params[1]" in str(e.value)
        ao.synchronize()
        for t in out:
            assert bool((t == 0xA5).all())
        after = L.Params()
        L.check(ao._lib.meao_get_params(ao._ctx, C.byref(after)), ao._ctx)
        assert bytes(before) == bytes(after)
        ao.execute_device([t.data_ptr() for t in dd], [t.data_ptr() for t in out])
        ao.synchronize()
        for f in range(n):
            assert np.array_equal(out[f].cpu().numpy(), oracle.run(depths[f], base, result_only=True)["result"]), f
    finally:
        ao.close()


# ---- which kernels the per-frame calls launch (rocprofv3 kernel trace of a child process)

TRACE_STRUCTURES = r"""
import dataclasses
import numpy as np
from oracle import oracle as O
from miniengineao_amd import _lib as L
from miniengineao_amd import synth
from tests import helpers as H
from tests.helpers import random_params


def run(w, h, n, debug=None, **cfg):
    base = dataclasses.replace(H.settings(O, w, h), **cfg)
    ao = H.component(base, max_batch=n, debug=debug)
    try:
        ao.render_batch([synth.make("S2", w, h, seed=5 + f) for f in range(n)], params=random_params(np.random.default_rng(n), w, h, n))
    finally:
        ao.close()


run(1920, 1080, 1)                                   # three-level nested blend, small render / final / downsample tiles
run(256, 160, 6, {L.DEBUG_NESTED_MAX_TILES: 0, L.DEBUG_BLEND_TALL_MIN_TILES: 1, L.DEBUG_RENDER_SMALL_MAX_TILES: 0,
                  L.DEBUG_FINAL_SMALL_MAX_TILES: 0})  # two-level, tall L2 -> L1, 128 x 32 render, 64 x 64 final
run(256, 160, 2, hq_levels=2)                        # Render.main (wide) + separate blend passes
"""

TRACE_PIPELINED = r"""
import dataclasses
import numpy as np
import torch
from oracle import oracle as O
from miniengineao_amd import _lib as L
from miniengineao_amd import synth
from tests import helpers as H
from tests.helpers import random_params

w, h, B = 384, 256, 4
ao = H.component(H.settings(O, w, h), max_batch=B, pipelined=True)
params = [random_params(np.random.default_rng(k), w, h, B) for k in range(3)]
announced2 = [dataclasses.replace(p, nearClipPlane=float(np.float32(p.nearClipPlane * 2))) for p in params[2]]
dev = torch.device("cuda", 0)
dd = [[torch.from_numpy(synth.make("S2", w, h, seed=10 * k + f)).to(dev) for f in range(B)] for k in range(3)]
out = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(B)]
for k in range(3):
    if k + 1 < 3:
        ao.prefetch_device([t.data_ptr() for t in dd[k + 1]], params=announced2 if k + 1 == 2 else params[k + 1])
    ao.execute_device([t.data_ptr() for t in dd[k]], [t.data_ptr() for t in out], params=params[k])
torch.cuda.synchronize(dev)
ao.close()
"""


def test_per_frame_calls_reach_every_launch_structure(tmp_path):
    k = H.kernel_trace(tmp_path, TRACE_STRUCTURES)
    for name in ("downsample_frames_kernel", "render_frames_kernel", "render_small_frames_kernel", "render_wide_frames_kernel",
                 "upsample_frames_kernel", "upsample_blend_tall_frames_kernel", "upsample_two_level_frames_kernel",
                 "upsample_three_level_frames_kernel", "upsample_final_frames_kernel", "upsample_final_small_frames_kernel"):
        assert k[name] > 0, (name, k)
    for shared in ("downsample_kernel", "render_kernel", "render_small_kernel", "render_wide_kernel", "render_with_composite_kernel",
                   "upsample_kernel", "upsample_blend_tall_kernel", "upsample_two_level_kernel", "upsample_three_level_kernel",
                   "upsample_final_kernel", "upsample_final_small_kernel"):
        assert k[shared] == 0, (shared, k)       # per-frame calls launch the per-frame forms only


def test_pipelined_per_frame_stream_kernels(tmp_path):
    k = H.kernel_trace(tmp_path, TRACE_PIPELINED)
    # step 0: own downsample + fused last kernel carrying batch 1; step 1: batch 1's pass reused + fused kernel carrying batch 2;
    # step 2: announced with another near plane -> its pass re-runs, plain last kernel
    assert k["upsample_final_with_next_downsample_frames_kernel"] == 2, k
    assert k["downsample_frames_kernel"] == 2, k
    assert k["upsample_final_frames_kernel"] + k["upsample_final_small_frames_kernel"] == 1, k
    assert k["upsample_final_with_next_downsample_kernel"] == 0 and k["downsample_kernel"] == 0, k
