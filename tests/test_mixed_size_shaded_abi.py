"""Shaded frames from mixed-size batches, the part that needs no GPU: the contracts the header states for
meao_composite_batch_extents / meao_execute_batch_extents_shaded / meao_pool_execute_batch_extents_shaded, what the C++ and
Python wrappers offer for them, and the argument checks that touch no device (meao_target_extent and the prototypes in every
mirror are tests/test_abi_mirrors.py)."""
import ctypes as C
import inspect
import os
import re

import pytest

from miniengineao_amd import _lib as L
from tests import abi_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_contracts_are_in_the_header():
    text = A.header_prose()
    for phrase in ("the call IS meao_composite_batch", "Each half classifies itself", "applies to packed frames too",
                   "8 x max_batch x 64 bytes", "chosen PER FRAME", "meao_composite_batch_extents, or shaded in the same call"):
        assert phrase in text, phrase


def test_cpp_and_csharp_mirrors():
    hpp = A.read(A.HPP_PATH)
    assert len(re.findall(r"\bvoid CompositeBatchExtents\(", hpp)) == 1
    assert len(re.findall(r"\bvoid RenderDeviceBatchExtentsShaded\(", hpp)) == 2           # the context class and the pool class
    assert "std::vector<meao_target_extent>" in hpp


def test_cpp_wrappers_compile(tmp_path):
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "meao.hpp"\n'
                   "void probe(MiniEngineAO::AmbientOcclusion &ao, MiniEngineAO::AmbientOcclusionPool &pool) {\n"
                   "  std::vector<meao_target_extent> e{{8, 8, 0, 0, 0}};\n"
                   "  ao.CompositeBatchExtents(MEAO_COMPOSITE_MULTIPLY, {nullptr}, {nullptr}, e);\n"
                   "  ao.RenderDeviceBatchExtentsShaded({nullptr}, {nullptr}, e, MEAO_COMPOSITE_MULTIPLY, {nullptr});\n"
                   "  pool.RenderDeviceBatchExtentsShaded({nullptr}, {nullptr}, e, MEAO_COMPOSITE_MULTIPLY, {nullptr}, MEAO_COLOR_RGBA8); }\n")
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_null_arguments_are_refused_without_a_device(meao_lib):
    one = (C.c_void_p * 1)(1)
    ext = (L.Extent * 1)()
    target = (L.TargetExtent * 1)()
    ext[0].width = ext[0].height = target[0].width = target[0].height = 8
    E = L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_composite_batch_extents(None, 0, 1, one, one, 0, None, target, None) == E
    assert meao_lib.meao_execute_batch_extents_shaded(None, 1, one, one, ext, None, 0, one, 0, None, None, None, None) == E
    assert meao_lib.meao_pool_execute_batch_extents_shaded(None, 1, one, one, ext, None, 0, one, 0, None, None, None) == E
    # a pool call with a null array is refused before the pool is looked at (the handle is never dereferenced)
    fake = C.c_void_p(1)
    assert meao_lib.meao_pool_execute_batch_extents_shaded(fake, 1, one, one, None, None, 0, one, 0, None, None, None) == E
    assert meao_lib.meao_pool_execute_batch_extents_shaded(fake, 1, one, one, ext, None, 0, None, 0, None, None, None) == E
    assert meao_lib.meao_pool_execute_batch_extents_shaded(fake, 1, None, one, ext, None, 0, one, 0, None, None, None) == E


def test_target_extents_array():
    from miniengineao_amd.ambient_occlusion import target_extents_array
    arr = target_extents_array([(33, 17), (400, 272, 512, 3264, 1700)], 2)
    assert [(e.width, e.height, e.ao_pitch, e.color_pitch, e.gbuffer0_pitch) for e in arr] == [(33, 17, 0, 0, 0), (400, 272, 512, 3264, 1700)]
    for bad in ([(33, 17)], [(33, 17), (1, 2, 3)], [(33, 17), (1, 2, 3, 4)], [(33, 17), (1, 2, 3, 4, 5, 6)]):
        with pytest.raises(ValueError):
            target_extents_array(bad, 2)


def test_python_signatures():
    from miniengineao_amd import AmbientOcclusion, AmbientOcclusionPool
    for cls in (AmbientOcclusion, AmbientOcclusionPool):
        sig = inspect.signature(cls.execute_shaded_device).parameters
        for name in ("extents", "color_pitches", "gbuffer0_pitches"):
            assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default is None, (cls, name)
    p = inspect.signature(AmbientOcclusion.composite_batch_device).parameters["extents"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
