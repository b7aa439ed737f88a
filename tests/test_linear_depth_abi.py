"""Linear view-space depth input (MEAO_DEPTH_LINEAR_F32 / _F16): the config checks and byte counts that need no device, the
Python dtype maps, and the linear kernels' compile-time resources against their raw-F32 twins."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from miniengineao_amd import _lib as L
from miniengineao_amd.ambient_occlusion import DEPTH_NUMPY, DEPTH_TORCH
from tests.kernel_inventory import HOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def config(fmt, w=640, h=360):
    cfg = L.Config()
    L.load().meao_default_config(C.byref(cfg))
    cfg.width, cfg.height, cfg.depth_format = w, h, fmt
    return cfg


def algorithmic_bytes(fmt):
    out = (C.c_uint64 * L.NUM_PASSES)()
    rc = L.load().meao_algorithmic_bytes(C.byref(config(fmt)), C.byref(out))
    return rc, list(out)


@pytest.mark.parametrize("fmt", [L.DEPTH_LINEAR_F32, L.DEPTH_LINEAR_F16])
def test_create_accepts_the_linear_formats(fmt):
    ctx = C.c_void_p()
    rc = L.load().meao_create(C.byref(config(fmt)), C.byref(ctx))
    try:
        assert rc != L.ERR_INVALID_ARGUMENT, L.load().meao_last_error(None)      # OK with a device, NO_DEVICE without one
    finally:
        if rc == L.OK:
            L.load().meao_destroy(ctx)


def test_create_rejects_the_next_value():
    ctx = C.c_void_p()
    assert L.load().meao_create(C.byref(config(6)), C.byref(ctx)) == L.ERR_INVALID_ARGUMENT
    assert algorithmic_bytes(6)[0] == L.ERR_INVALID_ARGUMENT


def test_algorithmic_bytes_count_the_element_size():
    w, h = 640, 360
    rc32, b32 = algorithmic_bytes(L.DEPTH_F32)
    rc_l32, lin32 = algorithmic_bytes(L.DEPTH_LINEAR_F32)
    rc_l16, lin16 = algorithmic_bytes(L.DEPTH_LINEAR_F16)
    assert rc32 == rc_l32 == rc_l16 == L.OK
    assert lin32 == b32
    assert lin16[0] == b32[0] - 2 * w * h and lin16[1:] == b32[1:]          # 2-byte texels in the downsample pass
    assert lin16 == algorithmic_bytes(L.DEPTH_F16)[1]


def test_python_dtype_maps():
    assert DEPTH_NUMPY[L.DEPTH_LINEAR_F32] is np.float32 and DEPTH_NUMPY[L.DEPTH_LINEAR_F16] is np.float16
    assert DEPTH_TORCH[L.DEPTH_LINEAR_F32] == "float32" and DEPTH_TORCH[L.DEPTH_LINEAR_F16] == "float16"
    assert DEPTH_NUMPY[L.DEPTH_F16] is np.uint16 and DEPTH_TORCH[L.DEPTH_F32] == "float32"       # the raw formats keep theirs
    assert set(DEPTH_NUMPY) == set(DEPTH_TORCH) == set(range(6))


@pytest.fixture(scope="module")
def rows():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here: the compile-time resource table cannot be produced")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         capture_output=True, text=True, check=True, cwd=ROOT, timeout=900)
    return {r["name"]: r for r in json.loads(out.stdout)}


# linear template -> (raw template, template arguments of the raw-F32 twin given the linear one's)
def twin(name):
    base, args = name.split("<", 1)
    args = [a.strip() for a in args.rstrip(">").split(",")]
    if base.startswith("downsample_linear"):
        return base.replace("_linear", "") + "<%s>" % ", ".join(args)
    if base.startswith("upsample_final_with_next_downsample_linear"):
        return base.replace("_linear", "") + "<%s>" % ", ".join(args)
    if base.startswith("upsample_final"):
        return base.replace("_linear", "") + "<%s>" % ", ".join(args[:3] + ["true"])
    return None


def test_linear_kernels_keep_the_raw_f32_resources(rows):
    linear = [n for n in rows if "linear" in n.split("<")[0] and twin(n)]
    assert len(linear) == 76, len(linear)
    assert not [n for n in linear if "pitched" in n]
    for name in linear:
        r, t = rows[name], rows[twin(name)]
        assert int(r["Occupancy [waves/SIMD]"]) >= int(t["Occupancy [waves/SIMD]"]), (name, r, t)
        assert int(r["LDS Size [bytes/block]"]) <= int(t["LDS Size [bytes/block]"]), (name, r, t)
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["AGPRs"]) == 0, (name, r)
    for name in linear:
        if twin(name) in HOT:                 # the linear instances of a hot kernel stay inside its VGPR budget
            assert int(rows[name]["VGPRs"]) <= HOT[twin(name)][1], (name, rows[name])
    assert [n for n in linear if twin(n) == "upsample_final_with_next_downsample_kernel<0, false, 0>"]
