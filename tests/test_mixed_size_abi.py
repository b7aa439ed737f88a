"""Mixed-size batches, the part that needs no GPU: meao_extent and the prototypes of meao_execute_batch_extents /
meao_pool_execute_batch_extents in include/meao.h, the exported symbols, and the Python, C++ and C# mirrors of the struct and the
calls."""
import ctypes as C
import inspect
import os
import re

from miniengineao_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "meao.h")).read()
NEW_CALLS = {"meao_execute_batch_extents": 7, "meao_pool_execute_batch_extents": 6}
# meao_extent: two int32 and two uint64, in this order -- 24 bytes, the pitches at offsets 8 and 16
FIELDS = [("width", "int32_t", 0), ("height", "int32_t", 4), ("depth_pitch", "uint64_t", 8), ("ao_pitch", "uint64_t", 16)]


def test_header_carries_the_struct_and_the_prototypes_and_the_abi_version_stays():
    for name, nargs in NEW_CALLS.items():
        m = re.search(r"MEAO_API\s+int32_t\s+%s\s*\((.*?)\);" % name, HEADER, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert "const meao_extent *extents" in m.group(1) and "const meao_params *params" in m.group(1), name
    body = re.search(r"typedef struct meao_extent \{(.*?)\} meao_extent;", HEADER, re.S)
    assert body
    declared = [(name, ctype) for ctype, names in re.findall(r"(u?int\d+_t)\s+([^;]+);", body.group(1)) for name in re.split(r",\s*", names)]
    assert declared == [(n, t) for n, t, _ in FIELDS]
    assert re.search(r"#define\s+MEAO_ABI_VERSION\s+7\b", HEADER) and L.ABI_VERSION == 7


def test_library_exports_the_calls(meao_lib):
    """(They fail here on a library without the feature: ctypes raises AttributeError for a missing symbol.)"""
    for name, nargs in NEW_CALLS.items():
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(meao_lib, name)
    assert meao_lib.meao_abi_version() == 7


def test_python_struct_mirror():
    assert C.sizeof(L.Extent) == 24
    assert [(n, getattr(L.Extent, n).offset, getattr(L.Extent, n).size) for n, _ in L.Extent._fields_] == \
        [(n, off, 4 if t == "int32_t" else 8) for n, t, off in FIELDS]
    for name in NEW_CALLS:
        assert C.POINTER(L.Extent) in L.SIGNATURES[name][1] and C.POINTER(L.Params) in L.SIGNATURES[name][1]


def test_cpp_and_csharp_mirrors():
    hpp = open(os.path.join(ROOT, "include", "meao.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "MeaoNative.cs")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b%s\(" % name, hpp), name
        m = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\((.*?)\);" % name, cs)
        assert m and len(m.group(1).split(",")) == NEW_CALLS[name] and "[In] MeaoExtent[] extents" in m.group(1), name
    for method in ("RenderBatchExtents", "RenderDeviceBatchExtents"):
        assert re.search(r"\b%s\(" % method, hpp), method
    # the C++ wrapper uses the C struct itself; the C# struct is sequential with the C fields in order
    assert "std::vector<meao_extent>" in hpp
    body = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*public struct MeaoExtent\s*\{(.*?)\}", cs, re.S)
    assert body
    cs_type = {"int32_t": "int", "uint64_t": "ulong"}
    assert re.findall(r"public (\w+) (\w+);", body.group(1)) == [(cs_type[t], n) for n, t, _ in FIELDS]


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
