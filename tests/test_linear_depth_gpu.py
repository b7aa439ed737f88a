"""Linear view-space depth input (MEAO_DEPTH_LINEAR_F32 / _F16) on the GPU.

Everything downstream of Linearize reads Linear01 depth only, so a linear frame equal to the Linearize of a raw frame must give the
raw frame's results bit for bit.  The reference: a raw frame d and its camera (far_clip a power of two); dist = Linearize(d) as
the oracle evaluates it (1 / fmaf(zp.x, d, zp.y), sky select; fmaf exact, in C); z = dist * far (exact).  A non-sky raw texel whose
dist is >= 1 is made a sky texel in d first; sky texels become far or +inf, alternating.  Then library(LINEAR, z) == oracle(d).
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import kernel_inventory as K
from tests.helpers import PASS_DOWNSAMPLE, compare
from tests.linear_depth import linearize, to_linear

pytestmark = pytest.mark.gpu

CAM_REV = synth.Camera(near=0.1, far=128.0, reversed_z=True)
CAM_CONV = synth.Camera(near=0.1, far=128.0, reversed_z=False)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def linearize_c():
    return linearize()


def check_ids(ao, want, ids, frame=0, checksums=False):
    for i in ids:
        g = ao.debug_buffer(i, frame=frame)
        if checksums:
            assert H.checksum(g) == H.checksum(want[H.NAMES[i]]), (i, frame)
        else:
            compare(g, want[H.NAMES[i]], H.NAMES[i])


def run_host(oracle, lin_c, frames, cam, fmt=L.DEPTH_LINEAR_F32, ids=(), checksums=False, nthreads=16, **kw):
    """frames: raw f32 frames of one size; one batched call through the HOST staging path."""
    h, w = frames[0].shape
    s = H.settings(oracle, w, h, cam=cam, **kw)
    pairs = [to_linear(lin_c, f, cam) for f in frames]
    ao = H.component(s, max_batch=len(frames), depth_format=fmt)
    try:
        zs = [z if fmt == L.DEPTH_LINEAR_F32 else z.astype(np.float16) for _, z in pairs]
        outs = ao.render_batch(zs)
        for f, (d, _) in enumerate(pairs):
            want = oracle.run(d, s, nthreads=nthreads, result_only=not ids)
            compare(outs[f], want["result"], "result")
            check_ids(ao, want, ids, frame=f, checksums=checksums)
    finally:
        ao.close()


ALL_IDS = list(range(1, 18))


def fixture_depth(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["depth"]


def test_sky_fixture_frame(oracle, linearize_c):
    d = fixture_depth("ref_s2_644x364_f16_rtne_convz_sky")
    run_host(oracle, linearize_c, [d], CAM_CONV, ids=ALL_IDS, ao_format=L.AO_F16, f16_rounding=L.F16_RTNE)
    run_host(oracle, linearize_c, [d], CAM_CONV, ids=[1, 2, 17], ao_format=L.AO_F16, f16_rounding=L.F16_RTZ_CLAMP)


def test_hostile_fixture_frame(oracle, linearize_c):
    d = fixture_depth("ref_s2h_516x260_hostile_r8")
    run_host(oracle, linearize_c, [d], CAM_REV, ids=ALL_IDS)


def test_1080p_s3_and_4k_s2(oracle, linearize_c):
    sponza = synth.Camera(near=0.01, far=128.0, fov_y_deg=30.0)
    run_host(oracle, linearize_c, [synth.atrium(1920, 1080, cam=sponza)], sponza, ids=ALL_IDS, checksums=True)
    run_host(oracle, linearize_c, [synth.make("S2", 3840, 2160)], CAM_REV, ids=ALL_IDS, checksums=True)


def test_batch_and_small_tiles(oracle, linearize_c):
    run_host(oracle, linearize_c, [synth.occluder_field(260, 36, seed=s, cam=CAM_REV) for s in range(3)], CAM_REV, ids=[1, 2, 10, 17])
    run_host(oracle, linearize_c, [synth.occluder_field(644, 364, seed=s, cam=CAM_REV) for s in range(4)], CAM_REV, ids=[2, 17])


@pytest.mark.parametrize("kw", [dict(ao_format=L.AO_R8, f16_rounding=L.F16_RTNE), dict(ao_format=L.AO_F16, f16_rounding=L.F16_RTZ_CLAMP),
                                dict(hq_levels=2), dict(sample_set=L.SAMPLES_EXHAUSTIVE), dict(single_pass_stereo=True)])
def test_variants(oracle, linearize_c, kw):
    run_host(oracle, linearize_c, [synth.occluder_field(322, 182, seed=11, cam=CAM_REV)], CAM_REV, ids=[1, 2, 17], **kw)


def test_linear_f16_equals_linear_f32_of_the_widened_values(oracle, linearize_c):
    w, h = 644, 364
    s = H.settings(oracle, w, h, cam=CAM_REV)
    _, z = to_linear(linearize_c, synth.occluder_field(w, h, seed=3, cam=CAM_REV), CAM_REV)
    z16 = z.astype(np.float16)
    a16 = H.component(s, depth_format=L.DEPTH_LINEAR_F16)
    a32 = H.component(s, depth_format=L.DEPTH_LINEAR_F32)
    try:
        r16 = a16.render(z16)
        r32 = a32.render(z16.astype(np.float32))
        assert np.array_equal(r16, r32)
        for i in (1, 2, 17):
            compare(a16.debug_buffer(i), a32.debug_buffer(i), H.NAMES[i])
    finally:
        a16.close()
        a32.close()


def test_linear01_input_equals_eye_depth_input(oracle, linearize_c):
    w, h = 322, 182
    for cam in (CAM_REV, CAM_CONV):
        _, z = to_linear(linearize_c, synth.occluder_field(w, h, seed=5, cam=cam), cam)
        eye = H.component(H.settings(oracle, w, h, cam=cam), depth_format=L.DEPTH_LINEAR_F32)
        unit = dataclasses.replace(cam, near=float(np.float32(cam.near) / np.float32(cam.far)), far=1.0)
        one = H.component(H.settings(oracle, w, h, cam=unit), depth_format=L.DEPTH_LINEAR_F32)
        try:
            assert np.array_equal(eye.render(z), one.render(z / np.float32(cam.far)))
        finally:
            eye.close()
            one.close()


def hostile_split(w, h, seed, even_even):
    """S2 with hostile raw texels only where (y, x) are both even (the level texels) or only elsewhere (odd texels)."""
    clean = synth.make("S2", w, h, seed=seed)
    d = H.hostile_frame(w, h, seed, cam=CAM_REV, density=0.02)
    yy, xx = np.mgrid[0:h, 0:w]
    ee = ((yy & 1) == 0) & ((xx & 1) == 0)
    keep = ee if even_even else ~ee
    return np.where(keep, d, clean).astype(np.float32)


def test_pipelined_fused_last_kernel_with_hostile_frames(oracle, linearize_c):
    w, h, n = 640, 360, 2
    s = H.settings(oracle, w, h, cam=CAM_REV)
    raws = [[synth.occluder_field(w, h, seed=10 * k + f, cam=CAM_REV) for f in range(n)] for k in range(3)]
    raws[1] = [hostile_split(w, h, 41, even_even=False), hostile_split(w, h, 42, even_even=True)]
    pairs = [[to_linear(linearize_c, d, CAM_REV) for d in step] for step in raws]
    ao = H.component(s, max_batch=n, pipelined=True, depth_format=L.DEPTH_LINEAR_F32)
    try:
        depth = [torch.from_numpy(np.stack([z for _, z in step])).cuda() for step in pairs]
        out = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(3)]
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        for k in range(3):
            if k == 1:
                ao.set_profiling(True)
            if k + 1 < 3:
                ao.prefetch_device([depth[k + 1][f].data_ptr() for f in range(n)])
            ao.execute_device([depth[k][f].data_ptr() for f in range(n)], [out[k][f].data_ptr() for f in range(n)], stream=stream)
            if k == 1:
                # frame 1: hostile level texels; frame 0's hostile texels are all odd ones, which the final pass tests per lane only
                assert ao.hostile_frames() == 0b10
        ms, samples = ao.pass_times_ms()
        assert samples == 2 and ms[PASS_DOWNSAMPLE] == 0, ms          # the carried passes ran inside the fused last kernel
        torch.cuda.synchronize()
        for k in range(3):
            for f, (d, _) in enumerate(pairs[k]):
                want = oracle.run(d, s, result_only=k != 2)
                compare(out[k][f].cpu().numpy(), want["result"], "result")
                if k == 2:
                    check_ids(ao, want, [2, 17], frame=f)
    finally:
        ao.close()


def test_per_frame_params_with_a_far_clip_per_frame(oracle, linearize_c):
    w, h, n = 640, 360, 3
    fars = [64.0, 128.0, 256.0]
    base = H.settings(oracle, w, h, cam=CAM_REV)
    ao = H.component(base, max_batch=n, pipelined=True, depth_format=L.DEPTH_LINEAR_F32)
    try:
        cams = [dataclasses.replace(CAM_REV, far=fa) for fa in fars]
        pairs = [to_linear(linearize_c, synth.occluder_field(w, h, seed=20 + f, cam=c), c) for f, c in enumerate(cams)]
        params = [FrameParams(farClipPlane=fa) for fa in fars]
        depth = torch.from_numpy(np.stack([z for _, z in pairs])).cuda()
        outs = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
        stream = torch.cuda.current_stream().cuda_stream
        ptrs = [depth[f].data_ptr() for f in range(n)]
        ao.prefetch_device(ptrs, params)
        ao.execute_device(ptrs, [outs[0][f].data_ptr() for f in range(n)], stream=stream, params=params)      # carries the next
        ao.execute_device(ptrs, [outs[1][f].data_ptr() for f in range(n)], stream=stream, params=params)      # consumes it
        torch.cuda.synchronize()
        for f, (d, _) in enumerate(pairs):
            sf = dataclasses.replace(base, far_clip=np.float32(fars[f]))
            want = oracle.run(d, sf)
            for o in outs:
                compare(o[f].cpu().numpy(), want["result"], "result")
            check_ids(ao, want, [1, 2, 6, 17], frame=f)
    finally:
        ao.close()


# A prefetched pass of linear frames is reused when each frame's s = RN(1 / far_clip) matches, whatever near_clip and reversed_z
# are (the levels depend on s alone); another far_clip reruns it.  The context's camera is CAM_REV; the consuming call brings
# its own, and its results must be the oracle's under that camera.
@pytest.mark.parametrize("change,reused", [("far", False), ("near", True), ("reversed_z", True)])
def test_prefetch_reuse_key_is_s(oracle, linearize_c, change, reused):
    w, h, n = 640, 360, 2
    cam_b = {"far": dataclasses.replace(CAM_REV, far=256.0), "near": dataclasses.replace(CAM_REV, near=0.2),
             "reversed_z": CAM_CONV}[change]
    s_b = H.settings(oracle, w, h, cam=cam_b)
    ao = H.component(H.settings(oracle, w, h, cam=CAM_REV), max_batch=n, pipelined=True, depth_format=L.DEPTH_LINEAR_F32)
    try:
        first = [to_linear(linearize_c, synth.occluder_field(w, h, seed=70 + f, cam=CAM_REV), CAM_REV) for f in range(n)]
        pairs = [to_linear(linearize_c, synth.occluder_field(w, h, seed=80 + f, cam=cam_b), cam_b) for f in range(n)]
        depth0 = torch.from_numpy(np.stack([z for _, z in first])).cuda()
        depth1 = torch.from_numpy(np.stack([z for _, z in pairs])).cuda()
        out = torch.zeros((2, n, h, w), dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ptrs1 = [depth1[f].data_ptr() for f in range(n)]
        ao.prefetch_device(ptrs1)                                  # announced under the context's camera (s = 1 / 128)
        ao.execute_device([depth0[f].data_ptr() for f in range(n)], [out[0, f].data_ptr() for f in range(n)], stream=stream)
        ao.set_profiling(True)
        params = [FrameParams(nearClipPlane=cam_b.near, farClipPlane=cam_b.far, usesReversedZBuffer=cam_b.reversed_z)] * n
        ao.execute_device(ptrs1, [out[1, f].data_ptr() for f in range(n)], stream=stream, params=params)
        ms, samples = ao.pass_times_ms()
        assert samples >= 1 and (ms[PASS_DOWNSAMPLE] == 0) == reused, (change, ms)
        torch.cuda.synchronize()
        for f, (d, _) in enumerate(pairs):
            want = oracle.run(d, s_b)
            compare(out[1, f].cpu().numpy(), want["result"], "result")
            check_ids(ao, want, [2, 6, 17], frame=f)
    finally:
        ao.close()


@pytest.mark.parametrize("fmt", [L.DEPTH_LINEAR_F32, L.DEPTH_LINEAR_F16])
@pytest.mark.parametrize("w,x0,extra", [(640, 0, 128), (644, 1, 3)])
def test_pitched_surfaces(oracle, linearize_c, fmt, w, x0, extra):
    h, n = 364, 2
    s = H.settings(oracle, w, h, cam=CAM_REV)
    pairs = [to_linear(linearize_c, synth.occluder_field(w, h, seed=30 + f, cam=CAM_REV), CAM_REV) for f in range(n)]
    tdt = torch.float32 if fmt == L.DEPTH_LINEAR_F32 else torch.float16
    surf = torch.full((n, h + 2, x0 + w + extra), float("nan"), dtype=tdt, device="cuda")
    for f, (_, z) in enumerate(pairs):
        surf[f, 1:1 + h, x0:x0 + w] = torch.from_numpy(z).to(tdt)
    out_surf = torch.full((n, h + 2, x0 + w + extra), 0xA5, dtype=torch.uint8, device="cuda")
    ao = H.component(s, max_batch=n, depth_format=fmt)
    try:
        ao.execute_tensors(surf[:, 1:1 + h, x0:x0 + w], out_surf[:, 1:1 + h, x0:x0 + w])
        torch.cuda.synchronize()
        o = out_surf.cpu().numpy()
        for f, (d, z) in enumerate(pairs):
            if fmt == L.DEPTH_LINEAR_F16:      # the widened f16 values through the f32 path
                ref = H.component(s, depth_format=L.DEPTH_LINEAR_F32)
                try:
                    want = ref.render(z.astype(np.float16).astype(np.float32))
                finally:
                    ref.close()
            else:
                want = oracle.run(d, s, result_only=True)["result"]
            assert np.array_equal(o[f, 1:1 + h, x0:x0 + w], want)
            mask = np.ones(o[f].shape, bool)
            mask[1:1 + h, x0:x0 + w] = False
            assert (o[f][mask] == 0xA5).all()
    finally:
        ao.close()


def test_pool_two_members(oracle, linearize_c):
    from miniengineao_amd import AmbientOcclusionPool
    w, h, n = 260, 36, 4
    s = H.settings(oracle, w, h, cam=CAM_REV)
    pool = AmbientOcclusionPool(w, h, [0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                                reversed_z=s.reversed_z, depth_format=L.DEPTH_LINEAR_F32)
    try:
        pairs = [to_linear(linearize_c, synth.occluder_field(w, h, seed=50 + f, cam=CAM_REV), CAM_REV) for f in range(n)]
        outs = pool.render_batch([z for _, z in pairs])
        for f, (d, _) in enumerate(pairs):
            compare(outs[f], oracle.run(d, s, result_only=True)["result"], "result")
    finally:
        pool.close()


TRACE = r"""
import numpy as np, torch
from miniengineao_amd import AmbientOcclusion, synth
from miniengineao_amd import _lib as L
w, h, n = 3840, 2160, 16
ao = AmbientOcclusion(w, h, max_batch=n, far_clip=128.0, pipelined=True, depth_format=FMT)
z = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(synth.make("S2", w, h), (n, h, w)))).cuda()
out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
dp, op = [z[f].data_ptr() for f in range(n)], [out[f].data_ptr() for f in range(n)]
s = torch.cuda.current_stream().cuda_stream
ao.prefetch_device(dp)
ao.execute_device(dp, op, stream=s)
ao.prefetch_device(dp)
ao.execute_device(dp, op, stream=s)
ao.execute_device(dp, op, stream=s)
torch.cuda.synchronize()
ao.close()
"""


def kernel_trace(tmp_path, fmt):
    """The child's meao kernels in start order, by template name."""
    return [K.split(n)[0] for n in H.kernel_trace(tmp_path / str(fmt), TRACE.replace("FMT", str(fmt))).short]


def test_kernel_trace_4k_pipelined_same_structure_as_raw_f32(tmp_path):
    raw = kernel_trace(tmp_path, L.DEPTH_F32)
    lin = kernel_trace(tmp_path, L.DEPTH_LINEAR_F32)
    assert "upsample_final_with_next_downsample_linear_kernel" in lin and "downsample_linear_kernel" in lin, lin
    assert not [k for k in lin if k in ("downsample_kernel", "upsample_final_kernel", "upsample_final_with_next_downsample_kernel")]
    assert [k.replace("_linear", "") for k in lin] == raw, (lin, raw)
