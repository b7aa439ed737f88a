"""Mixed-size batches, the part that needs no GPU: what the C++ and Python wrappers offer for meao_execute_batch_extents /
meao_pool_execute_batch_extents, and the null-argument checks (meao_extent and the prototypes in every mirror are
tests/test_abi_mirrors.py)."""
import ctypes as C
import inspect
import re

from miniengineao_amd import _lib as L
from tests import abi_model as A


def test_cpp_and_csharp_mirrors():
    hpp = A.read(A.HPP_PATH)
    for method in ("RenderBatchExtents", "RenderDeviceBatchExtents"):
        assert re.search(r"\b%s\(" % method, hpp), method
    assert "std::vector<meao_extent>" in hpp                 # the C++ wrapper uses the C struct itself


def test_null_arguments_are_refused_without_a_device(meao_lib):
    one = (C.c_void_p * 1)(1)
    ext = (L.Extent * 1)()
    ext[0].width = ext[0].height = 8
    assert meao_lib.meao_execute_batch_extents(None, 1, one, one, ext, None, None) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_execute_batch_extents(None, 1, one, one, ext, None) == L.ERR_INVALID_ARGUMENT


def test_python_signatures():
    from miniengineao_amd import AmbientOcclusion, AmbientOcclusionPool
    from miniengineao_amd.ambient_occlusion import extents_array
    for cls in (AmbientOcclusion, AmbientOcclusionPool):
        p = inspect.signature(cls.execute_device).parameters["extents"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, cls
    arr = extents_array([(33, 17), (400, 272, 1700, 512)], 2)
    assert [(e.width, e.height, e.depth_pitch, e.ao_pitch) for e in arr] == [(33, 17, 0, 0), (400, 272, 1700, 512)]
    for bad in ([(33, 17)], [(33, 17), (1, 2, 3)]):
        try:
            extents_array(bad, 2)
        except ValueError:
            continue
        raise AssertionError(bad)
