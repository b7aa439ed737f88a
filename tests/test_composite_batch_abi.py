"""meao_composite_batch, meao_execute_batch_shaded and meao_pool_execute_batch_shaded: the contracts the header states, the C#
wrapper and the Python signatures, what needs no device of their argument checks, and the rule that the batched form lives
inside composite_kernel<0|1>: no new instantiation, the resources of the two kernels as they were."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import pytest

from miniengineao_amd import _lib as L
from tests import abi_model as A
from tests import kernel_inventory as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["meao_composite_batch", "meao_execute_batch_shaded", "meao_pool_execute_batch_shaded"])
def test_entry_point_in_the_header(name):
    """Where the feature's arguments sit (the whole prototype, with its types and count, is pinned by tests/abi_snapshot.json)."""
    args = A.prototype(name)
    at = args.index("int32_t color_format")
    assert args[at - 1].endswith("color") and args[at + 1] == "uint64_t color_pitch"         # inserted after `color`
    for pitch in ("uint64_t ao_pitch", "uint64_t color_pitch", "uint64_t gbuffer0_pitch"):
        assert pitch in args, (name, pitch)
    assert ("meao_stream stream" in args) == (not name.startswith("meao_pool")), args
    if "shaded" in name:
        assert "uint64_t depth_pitch" in args and "const meao_params *params" in args


def test_the_contracts_are_in_the_header():
    text = A.header_prose()
    for phrase in ("ONE composite_kernel launch", "before anything is enqueued", "must not overlap", "neither run nor disturbed",
                   "meao_composite_pending is unchanged"):
        assert phrase in text, phrase


@pytest.mark.parametrize("name", ["meao_composite_batch", "meao_execute_batch_shaded"])
def test_entry_point_in_every_binding(name):
    """(The imports, signatures and the C++ wrapper's calls are tests/test_abi_mirrors.py.)  The C# wrapper calls it."""
    assert "Meao.%s(" % name in open(os.path.join(ROOT, "bindings", "csharp", "AmbientOcclusionOverMeao.cs")).read()


def test_entry_points_reject_null_handles(meao_lib):
    ptr = (C.c_void_p * 1)(None)
    E = L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_composite_batch(None, 0, 1, ptr, 0, ptr, 2, 0, None, 0, None) == E
    assert meao_lib.meao_execute_batch_shaded(None, 1, ptr, 0, ptr, 0, None, 0, ptr, 2, 0, None, 0, None) == E
    assert meao_lib.meao_pool_execute_batch_shaded(None, 1, ptr, 0, ptr, 0, None, 0, ptr, 2, 0, None, 0) == E


def test_python_mirrors_keep_the_old_signatures():
    import inspect
    from miniengineao_amd import AmbientOcclusion, AmbientOcclusionPool
    sig = inspect.signature(AmbientOcclusion.execute_tensors).parameters
    assert list(sig)[:4] == ["self", "depth", "out", "params"] and sig["color"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("color", "gbuffer0", "mode", "color_format"))
    sig = inspect.signature(AmbientOcclusion.composite_tensors).parameters
    assert list(sig)[:7] == ["self", "ao", "color", "gbuffer0", "mode", "enqueue", "color_format"] and sig["batched"].default is False
    assert sig["enqueue"].default is False
    for cls in (AmbientOcclusion, AmbientOcclusionPool):
        assert callable(getattr(cls, "execute_shaded_device"))
    assert callable(AmbientOcclusion.composite_batch_device)


# ---- the kernels: nothing new, the two that changed inside what they had

COMPOSITE_KERNELS = {"composite_kernel<0>", "composite_kernel<1>"} | {
    "render_with_composite_kernel<%s, %s, %s>" % col for col in K.COLUMNS}


@pytest.fixture(scope="module")
def rows():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc here: the compile-time resource table cannot be produced")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "--json"],
                         capture_output=True, text=True, check=True, cwd=ROOT, timeout=900)
    return {r["name"]: r for r in json.loads(out.stdout)}


def test_no_new_kernel_instantiation(rows):
    """The library's inventory (tests/kernel_inventory.py, what the coverage tests launch name by name) is what the sources compile
    to, and the kernels that composite are the eight there were: the batched form added none."""
    names = K.instantiations()
    assert {n for n in names if "composite" in n} == COMPOSITE_KERNELS
    assert set(names) == set(rows), sorted(set(names) ^ set(rows))
    assert len(names) == len(set(names))


@pytest.mark.parametrize("name", ["composite_kernel<0>", "composite_kernel<1>"])
def test_composite_kernels_keep_their_resources(rows, name):
    r = rows[name]
    assert int(r["Occupancy [waves/SIMD]"]) == 8, r
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and r["Dynamic Stack"] == "False", r
    assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["LDS Size [bytes/block]"]) == 0, r
    assert int(r["VGPRs"]) <= 64 and int(r["AGPRs"]) == 0, r       # (37 / 38 before and after the batched form)
