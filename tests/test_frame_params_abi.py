"""Per-frame parameters (meao_execute_batch_params and friends): the null-argument checks, the per-frame kernels' compile-time
resources against their shared forms, and FrameParams -> meao_params (no device needed)."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from miniengineao_amd.frame_params import params_array, to_params
from tests import abi_model as A
from tests.kernel_inventory import HOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["meao_execute_batch_params", "meao_prefetch_batch_params",
                                  "meao_pool_execute_batch_params", "meao_pool_prefetch_batch_params"])
def test_entry_point_everywhere(name):
    """Every per-frame form takes one meao_params per frame, as its last argument before the stream (types, counts and the three
    mirrors of the whole prototype are tests/test_abi_mirrors.py)."""
    args = A.prototype(name)
    assert "const meao_params *params" in args
    assert [a for a in args if a != "meao_stream stream"][-1] == "const meao_params *params"


def test_entry_points_reject_null_params(meao_lib):
    ptr = (C.c_void_p * 1)(None)
    assert meao_lib.meao_execute_batch_params(None, 1, ptr, L.MEM_DEVICE, ptr, L.MEM_DEVICE, None, None) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_prefetch_batch_params(None, 1, ptr, None) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_execute_batch_params(None, 1, ptr, L.MEM_DEVICE, ptr, L.MEM_DEVICE, None) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_prefetch_batch_params(None, 1, ptr, None) == L.ERR_INVALID_ARGUMENT


# ---- per-frame kernels: a form for every shared hot kernel, no worse occupancy / VGPRs / LDS, no scratch

# shared hot kernel -> its per-frame form (a composite waiting for a per-frame call is flushed as its own launch: the
# render_with_composite_kernel slot is taken by the plain per-frame render kernel)
PER_FRAME = {
    "render_kernel": "render_frames_kernel",
    "render_with_composite_kernel": "render_frames_kernel",
    "upsample_final_kernel": "upsample_final_frames_kernel",
    "upsample_final_with_next_downsample_kernel": "upsample_final_with_next_downsample_frames_kernel",
    "upsample_kernel": "upsample_frames_kernel",
    "upsample_two_level_kernel": "upsample_two_level_frames_kernel",
    "downsample_kernel": "downsample_frames_kernel",
}


def per_frame_name(shared):
    base, args = shared.split("<", 1)
    if base == "render_with_composite_kernel":
        args = args[:-1] + ", false>"          # render_kernel<AOFMT, RTNE, DIV, EXH = false>
    return PER_FRAME[base] + "<" + args


@pytest.fixture(scope="module")
def rows():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here: the compile-time resource table cannot be produced")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         capture_output=True, text=True, check=True, cwd=ROOT, timeout=900)
    return {r["name"]: r for r in json.loads(out.stdout)}


@pytest.mark.parametrize("shared", sorted(HOT))
@pytest.mark.parametrize("aofmt", ["0", "1"])
def test_per_frame_forms_keep_the_budget(rows, shared, aofmt):
    shared = shared.replace("<0, ", "<%s, " % aofmt, 1) if "<0, " in shared else shared
    s, p = rows[shared], rows.get(per_frame_name(shared))
    assert p is not None, per_frame_name(shared)
    assert int(p["Occupancy [waves/SIMD]"]) >= int(s["Occupancy [waves/SIMD]"]), (s, p)
    assert int(p["VGPRs"]) <= int(s["VGPRs"]) and int(p["AGPRs"]) == 0, (s, p)
    assert int(p["LDS Size [bytes/block]"]) <= int(s["LDS Size [bytes/block]"]), (s, p)


def test_no_per_frame_kernel_uses_scratch(rows):
    pf = {n: r for n, r in rows.items() if "_frames_kernel" in n}
    assert len(pf) >= 60, len(pf)
    bad = [n for n, r in pf.items() if int(r["ScratchSize [bytes/lane]"]) or int(r["VGPRs Spill"]) or r["Dynamic Stack"] != "False"]
    assert not bad, bad


# ---- FrameParams -> meao_params

def base_params():
    p = L.Params()
    p.struct_size = C.sizeof(L.Params)
    p.noise_filter_tolerance, p.blur_tolerance, p.upsample_tolerance = -1.0, -4.6, -12.0
    p.thickness_modifier, p.intensity = 2.0, 0.75
    p.near_clip, p.far_clip, p.proj00, p.reversed_z, p.single_pass_stereo = 0.3, 1000.0, 0.97, 1, 0
    return p


def test_unset_fields_take_the_instance_values():
    b = base_params()
    p = to_params(FrameParams(), b)
    assert bytes(p) == bytes(b)


def test_every_field_maps_to_its_c_field():
    b = base_params()
    fp = FrameParams(nearClipPlane=0.05, farClipPlane=5e4, projection00=1.5, usesReversedZBuffer=False,
                     singlePassStereoEnabled=True, intensity=2.5, thicknessModifier=4.0, noiseFilterTolerance=-6.0,
                     blurTolerance=-2.0, upsampleTolerance=-3.0)
    p = to_params(fp, b)
    want = dict(near_clip=0.05, far_clip=5e4, proj00=1.5, reversed_z=0, single_pass_stereo=1, intensity=2.5,
                thickness_modifier=4.0, noise_filter_tolerance=-6.0, blur_tolerance=-2.0, upsample_tolerance=-3.0)
    for k, v in want.items():
        assert getattr(p, k) == pytest.approx(v), k
    assert p.struct_size == C.sizeof(L.Params)
    assert b.near_clip == pytest.approx(0.3)       # the instance's block is not changed


def test_params_array_one_entry_per_frame():
    b = base_params()
    arr = params_array([FrameParams(intensity=1.5), None], 2, b)
    assert arr[0].intensity == 1.5 and arr[1].intensity == 0.75 and arr[1].near_clip == pytest.approx(0.3)
    with pytest.raises(ValueError):
        params_array([FrameParams()], 2, b)


def test_python_methods_take_params():
    import inspect
    from miniengineao_amd.ambient_occlusion import AmbientOcclusion, AmbientOcclusionPool
    for cls in (AmbientOcclusion, AmbientOcclusionPool):
        for m in ("render_batch", "execute_device", "prefetch_device"):
            sig = inspect.signature(getattr(cls, m))
            assert "params" in sig.parameters and sig.parameters["params"].default is None, (cls, m)
