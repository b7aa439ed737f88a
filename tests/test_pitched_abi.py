"""Row-pitched surfaces (meao_execute_batch_pitched and friends): argument checks that need no device, the tensor -> (pointer,
pitch) helper behind AmbientOcclusion.execute_tensors, and the pitched kernels' compile-time resources against their packed
forms."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.surfaces import frame_pointers, packed_pitch
from tests import abi_model as A
from tests.kernel_inventory import HOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["meao_execute_batch_pitched", "meao_prefetch_batch_pitched",
                                  "meao_pool_execute_batch_pitched", "meao_pool_prefetch_batch_pitched"])
def test_entry_point_everywhere(name):
    """Every pitched form takes the depth pitch in bytes and optional per-frame parameters (types, counts and the three mirrors of
    the whole prototype are tests/test_abi_mirrors.py)."""
    args = A.prototype(name)
    assert "uint64_t depth_pitch" in args and "const meao_params *params" in args
    assert ("uint64_t ao_pitch" in args) == ("execute" in name)


def test_entry_points_reject_null_arguments(meao_lib):
    ptr = (C.c_void_p * 1)(None)
    E = L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_execute_batch_pitched(None, 1, ptr, 0, L.MEM_DEVICE, ptr, 0, L.MEM_DEVICE, None, None) == E
    assert meao_lib.meao_prefetch_batch_pitched(None, 1, ptr, 0, None) == E
    assert meao_lib.meao_pool_execute_batch_pitched(None, 1, ptr, 0, L.MEM_DEVICE, ptr, 0, L.MEM_DEVICE, None) == E
    assert meao_lib.meao_pool_prefetch_batch_pitched(None, 1, ptr, 0, None) == E


# ---- frame_pointers (execute_tensors): crops, batch slices, rejected layouts -- on CPU tensors

def test_crop_of_a_batch_gives_the_surface_pitch():
    big = torch.zeros((4, 50, 70), dtype=torch.float32)
    crop = big[1:3, 5:45, 3:63]
    ptrs, pitch = frame_pointers(crop, 40, 60, torch.float32)
    assert pitch == 70 * 4
    base = big.data_ptr()
    assert ptrs == [base + ((1 + f) * 50 * 70 + 5 * 70 + 3) * 4 for f in range(2)]


def test_list_of_frames_and_any_batch_stride():
    a = torch.zeros((100, 64), dtype=torch.uint8)
    frames = [a[0:10, 0:20], a[37:47, 5:25]]
    ptrs, pitch = frame_pointers(frames, 10, 20, torch.uint8, "out")
    assert pitch == 64 and ptrs == [a.data_ptr(), a.data_ptr() + 37 * 64 + 5]
    packed = torch.zeros((3, 10, 20), dtype=torch.float16)
    ptrs, pitch = frame_pointers(packed, 10, 20, torch.float16)
    assert pitch == 40 and packed_pitch(pitch, 20, 2) == 0 and packed_pitch(64, 20, 1) == 64


def test_rejected_layouts():
    big = torch.zeros((2, 40, 60), dtype=torch.float32)
    with pytest.raises(ValueError, match="contiguous"):
        frame_pointers(big[:, :, ::2], 40, 30, torch.float32)
    with pytest.raises(ValueError, match="row strides"):
        frame_pointers([big[0], torch.zeros((40, 80))[:, :60]], 40, 60, torch.float32)
    with pytest.raises(ValueError, match="dtype"):
        frame_pointers(big, 40, 60, torch.float16)
    with pytest.raises(ValueError, match="shape"):
        frame_pointers(big, 40, 61, torch.float32)
    with pytest.raises(ValueError, match="contiguous"):
        frame_pointers(big.transpose(1, 2), 60, 40, torch.float32)


def test_every_frame_must_be_on_the_given_device():
    a, b = torch.zeros((40, 60)), torch.zeros((40, 60), device="meta")
    assert frame_pointers([a, a], 40, 60, torch.float32, device=torch.device("cpu"))[1] == 240
    with pytest.raises(ValueError, match=r"depth\[1\]: on meta"):
        frame_pointers([a, b], 40, 60, torch.float32, device=torch.device("cpu"))


# ---- pitched kernels: a form for every packed kernel that addresses caller memory, same occupancy, inside HOT, no scratch

PITCHED = {
    "upsample_final_kernel<0, false, 0, true>": "upsample_final_pitched_kernel<0, false, 0, true>",
    "upsample_final_with_next_downsample_kernel<0, false, 0>": "upsample_final_with_next_downsample_pitched_kernel<0, false, 0>",
    "downsample_kernel<true, 0, 2>": "downsample_pitched_kernel<true, 0, 2>",
}
FORMS = {  # packed kernel template -> pitched template (every instantiation of the packed one must have its pitched twin)
    "downsample_kernel": "downsample_pitched_kernel",
    "downsample_frames_kernel": "downsample_pitched_frames_kernel",
    "upsample_final_kernel": "upsample_final_pitched_kernel",
    "upsample_final_small_kernel": "upsample_final_small_pitched_kernel",
    "upsample_final_frames_kernel": "upsample_final_pitched_frames_kernel",
    "upsample_final_small_frames_kernel": "upsample_final_small_pitched_frames_kernel",
    "upsample_final_with_next_downsample_kernel": "upsample_final_with_next_downsample_pitched_kernel",
    "upsample_final_with_next_downsample_frames_kernel": "upsample_final_with_next_downsample_pitched_frames_kernel",
}


@pytest.fixture(scope="module")
def rows():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here: the compile-time resource table cannot be produced")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         capture_output=True, text=True, check=True, cwd=ROOT, timeout=900)
    return {r["name"]: r for r in json.loads(out.stdout)}


def test_every_packed_form_has_a_pitched_twin_with_its_occupancy(rows):
    pairs = 0
    for name, r in rows.items():
        base = name.split("<", 1)[0]
        if base not in FORMS:
            continue
        twin = rows.get(FORMS[base] + name[len(base):])
        assert twin is not None, name
        assert int(twin["Occupancy [waves/SIMD]"]) >= int(r["Occupancy [waves/SIMD]"]), (name, twin)
        assert int(twin["LDS Size [bytes/block]"]) <= int(r["LDS Size [bytes/block]"]), (name, twin)
        pairs += 1
    assert pairs == sum(1 for n in rows if "pitched" in n) == 76


@pytest.mark.parametrize("packed", sorted(PITCHED))
def test_pitched_hot_kernels_keep_the_budget(rows, packed):
    waves, vgprs, lds = HOT[packed]
    for fmt in ("<0, ", "<1, ") if packed.startswith("upsample") else ("<",):
        r = rows[PITCHED[packed].replace("<0, ", fmt, 1)]
        assert int(r["Occupancy [waves/SIMD]"]) >= waves and int(r["VGPRs"]) <= vgprs and int(r["AGPRs"]) == 0, r
        assert int(r["LDS Size [bytes/block]"]) <= lds, r


def test_no_pitched_kernel_uses_scratch(rows):
    bad = [n for n, r in rows.items() if "pitched" in n and
           (int(r["ScratchSize [bytes/lane]"]) or int(r["VGPRs Spill"]) or r["Dynamic Stack"] != "False")]
    assert not bad, bad
