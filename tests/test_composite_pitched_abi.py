"""The composite into row-pitched surfaces (meao_composite_pitched, meao_composite_enqueue_pitched,
meao_pool_composite_enqueue_pitched): argument checks that need no device, the tensor -> (pointer, pitch) helper behind
composite_tensors, and the rule that the feature lives in the kernels that already composite: no new instantiation, and the six
carrying kernels inside the budget of tests/test_kernel_resources.py."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.surfaces import composite_surfaces, frame_pointers
from tests import abi_model as A
from tests import kernel_inventory as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSITE_KERNELS = {"composite_kernel<0>", "composite_kernel<1>"} | {
    "render_with_composite_kernel<%d, %s, %d>" % (fmt, rtne, div)
    for fmt in (0, 1) for rtne, div in (("false", 0), ("false", 1), ("true", 1))}


def test_the_header_no_longer_says_the_composite_is_packed_only():
    assert "meao_composite* and meao_pool_gather_to_device take" not in A.header_prose()
    assert "meao_pool_gather_to_device takes tightly packed surfaces only" in A.header_prose()


def test_entry_points_reject_a_null_context(meao_lib):
    ptr = (C.c_void_p * 1)(None)
    E = L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_composite_pitched(None, 0, None, 0, None, 0, None, 0, L.MEM_DEVICE, None) == E
    assert meao_lib.meao_composite_enqueue_pitched(None, 0, 1, ptr, 0, ptr, 0, None, 0) == E
    assert meao_lib.meao_pool_composite_enqueue_pitched(None, 0, 1, ptr, 0, ptr, 0, None, 0) == E


# ---- composite_tensors: pointers and pitches of crops, on CPU tensors

def test_crops_of_larger_targets_give_their_pitches():
    h, w = 40, 60
    ao = torch.zeros((3, 50, 71), dtype=torch.uint8)
    color = torch.zeros((3, 48, 66, 4), dtype=torch.float16)
    gbuf = torch.zeros((3, 44, 64, 4), dtype=torch.uint8)
    a, ap, c, cp, g, gp = composite_surfaces(ao[:, 5:5 + h, 3:3 + w], color[:, 2:2 + h, 1:1 + w, :], gbuf[:, 4:4 + h, 2:2 + w, :],
                                             h, w, torch.uint8)
    assert (ap, cp, gp) == (71, 66 * 8, 64 * 4)
    assert a == [ao.data_ptr() + f * 50 * 71 + 5 * 71 + 3 for f in range(3)]
    assert c == [color.data_ptr() + ((f * 48 + 2) * 66 + 1) * 8 for f in range(3)]
    assert g == [gbuf.data_ptr() + ((f * 44 + 4) * 64 + 2) * 4 for f in range(3)]


def test_packed_tensors_lists_and_no_gbuffer0():
    h, w = 10, 20
    ao = [torch.zeros((h, w), dtype=torch.float16) for _ in range(2)]
    color = torch.zeros((2, h, w, 4), dtype=torch.int16)
    a, ap, c, cp, g, gp = composite_surfaces(ao, color, None, h, w, torch.float16)
    assert (ap, cp, g, gp) == (0, 0, None, 0)                       # tightly packed: the pitch-0 entry points
    assert a == [t.data_ptr() for t in ao] and c == [color[f].data_ptr() for f in range(2)]
    big = torch.zeros((64, 30, 4), dtype=torch.int16)
    _, pitch = frame_pointers([big[0:h, 0:w], big[20:20 + h, 5:5 + w]], h, w, torch.int16, "color", channels=4)
    assert pitch == 30 * 8


def test_frame_pointers_without_channels_is_unchanged():
    big = torch.zeros((4, 50, 70), dtype=torch.float32)
    ptrs, pitch = frame_pointers(big[1:3, 5:45, 3:63], 40, 60, torch.float32)
    assert pitch == 280 and ptrs == [big.data_ptr() + ((1 + f) * 50 * 70 + 5 * 70 + 3) * 4 for f in range(2)]


def test_rejected_layouts():
    h, w = 12, 16
    ao = torch.zeros((2, h, w), dtype=torch.uint8)
    color = torch.zeros((2, h, w, 4), dtype=torch.int16)

    def call(a=ao, c=color, g=None):
        return composite_surfaces(a, c, g, h, w, torch.uint8)
    with pytest.raises(ValueError, match="channels of a texel"):
        call(c=torch.zeros((2, h, w, 8), dtype=torch.int16)[..., ::2])
    with pytest.raises(ValueError, match="texels of a row"):
        call(c=torch.zeros((2, h, 2 * w, 4), dtype=torch.int16)[:, :, ::2, :])
    with pytest.raises(ValueError, match="row strides"):
        call(c=[color[0], torch.zeros((h, w + 3, 4), dtype=torch.int16)[:, :w, :]])
    with pytest.raises(ValueError, match="dtype"):
        call(c=color.to(torch.float32))
    assert call(c=color.view(torch.float16))[2] == call()[2]        # int16 and float16 are the two colour dtypes
    if hasattr(torch, "uint16"):
        with pytest.raises(ValueError, match="dtype"):
            call(c=color.view(torch.uint16))
    with pytest.raises(ValueError, match="dtype"):
        call(g=torch.zeros((2, h, w, 4), dtype=torch.int8))
    with pytest.raises(ValueError, match="shape"):
        call(c=torch.zeros((2, h, w, 3), dtype=torch.int16))
    with pytest.raises(ValueError, match=r"\(N, H, W, 4\)"):
        call(c=color[0])
    with pytest.raises(ValueError, match="frames"):
        call(c=color[:1])
    with pytest.raises(ValueError, match="frames"):
        call(g=torch.zeros((3, h, w, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="contiguous"):
        call(a=torch.zeros((2, h, 2 * w), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(c=torch.zeros((2, w, h, 4), dtype=torch.int16).transpose(1, 2))


# ---- the kernels: the eight that composite, nothing new, the carrying ones inside their budget

def test_no_new_composite_instantiation():
    names = K.instantiations()
    assert {n for n in names if "composite" in n} == COMPOSITE_KERNELS
    assert len(names) == 359


@pytest.fixture(scope="module")
def rows():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here: the compile-time resource table cannot be produced")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         capture_output=True, text=True, check=True, cwd=ROOT, timeout=900)
    return {r["name"]: r for r in json.loads(out.stdout)}


@pytest.mark.parametrize("name", sorted(n for n in COMPOSITE_KERNELS if n.startswith("render")))
def test_carrying_kernels_keep_the_budget(rows, name):
    r = rows[name]
    assert int(r["Occupancy [waves/SIMD]"]) >= 8 and int(r["VGPRs"]) <= 64 and int(r["AGPRs"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) <= 40960, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and r["Dynamic Stack"] == "False", r
