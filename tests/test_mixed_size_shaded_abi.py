"""Shaded frames from mixed-size batches, the part that needs no GPU: meao_target_extent and the prototypes of
meao_composite_batch_extents / meao_execute_batch_extents_shaded / meao_pool_execute_batch_extents_shaded in include/meao.h, the
exported symbols, the Python, C++ and C# mirrors of the struct and the calls, and the argument checks that touch no device."""
import ctypes as C
import inspect
import os
import re

import pytest

from miniengineao_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "meao.h")).read()
NEW_CALLS = {"meao_composite_batch_extents": 9, "meao_execute_batch_extents_shaded": 13, "meao_pool_execute_batch_extents_shaded": 12}
# meao_target_extent: two int32 and three uint64, in this order -- 32 bytes, the pitches at offsets 8, 16 and 24
FIELDS = [("width", "int32_t", 0), ("height", "int32_t", 4), ("ao_pitch", "uint64_t", 8), ("color_pitch", "uint64_t", 16),
          ("gbuffer0_pitch", "uint64_t", 24)]


def prototype(name):
    m = re.search(r"MEAO_API\s+int32_t\s+%s\s*\((.*?)\);" % name, HEADER, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_carries_the_struct_and_the_prototypes_and_the_abi_version_stays():
    for name, nargs in NEW_CALLS.items():
        assert len(prototype(name)) == nargs, name
    args = prototype("meao_composite_batch_extents")
    assert "const meao_target_extent *extents" in args and "int32_t color_format" in args and args[-1] == "meao_stream stream"
    for name in ("meao_execute_batch_extents_shaded", "meao_pool_execute_batch_extents_shaded"):
        args = prototype(name)
        for arg in ("const meao_extent *extents", "const meao_params *params", "const uint64_t *color_pitch",
                    "const uint64_t *gbuffer0_pitch", "int32_t color_format"):
            assert arg in args, (name, arg)
        assert ("meao_stream stream" in args) == (not name.startswith("meao_pool")), args
    body = re.search(r"typedef struct meao_target_extent \{(.*?)\} meao_target_extent;", HEADER, re.S)
    assert body
    plain = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    declared = [(name, ctype) for ctype, names in re.findall(r"(u?int\d+_t)\s+([^;]+);", plain) for name in re.split(r",\s*", names.strip())]
    assert declared == [(n, t) for n, t, _ in FIELDS]
    assert re.search(r"#define\s+MEAO_ABI_VERSION\s+7\b", HEADER) and L.ABI_VERSION == 7


def test_the_contracts_are_in_the_header():
    text = " ".join(HEADER.split())
    for phrase in ("the call IS meao_composite_batch", "Each half classifies itself", "applies to packed frames too",
                   "8 x max_batch x 64 bytes", "chosen PER FRAME", "meao_composite_batch_extents, or shaded in the same call"):
        assert phrase in text, phrase


def test_library_exports_the_calls(meao_lib):
    """(They fail here on a library without the feature: ctypes raises AttributeError for a missing symbol.)"""
    for name, nargs in NEW_CALLS.items():
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert getattr(meao_lib, name)
    assert meao_lib.meao_abi_version() == 7


def test_python_struct_mirror():
    assert C.sizeof(L.TargetExtent) == 32
    assert [(n, getattr(L.TargetExtent, n).offset, getattr(L.TargetExtent, n).size) for n, _ in L.TargetExtent._fields_] == \
        [(n, off, 4 if t == "int32_t" else 8) for n, t, off in FIELDS]
    assert C.POINTER(L.TargetExtent) in L.SIGNATURES["meao_composite_batch_extents"][1]
    for name in ("meao_execute_batch_extents_shaded", "meao_pool_execute_batch_extents_shaded"):
        args = L.SIGNATURES[name][1]
        assert C.POINTER(L.Extent) in args and C.POINTER(L.Params) in args and args.count(C.POINTER(C.c_uint64)) == 2, name


def test_cpp_and_csharp_mirrors():
    hpp = open(os.path.join(ROOT, "include", "meao.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "MeaoNative.cs")).read()
    for name, nargs in NEW_CALLS.items():
        assert re.search(r"\b%s\(" % name, hpp), name
        m = re.search(r"\[DllImport\(Lib\)\] public static extern int %s\((.*?)\);" % name, cs)
        assert m and len(m.group(1).split(",")) == nargs and "int color_format" in m.group(1), name
    assert "[In] MeaoTargetExtent[] extents" in cs
    for name in ("meao_execute_batch_extents_shaded", "meao_pool_execute_batch_extents_shaded"):
        m = re.search(r"extern int %s\((.*?)\);" % name, cs)
        assert "[In] MeaoExtent[] extents" in m.group(1) and "[In] ulong[] color_pitch" in m.group(1) and "[In] ulong[] gbuffer0_pitch" in m.group(1)
    assert len(re.findall(r"\bvoid CompositeBatchExtents\(", hpp)) == 1
    assert len(re.findall(r"\bvoid RenderDeviceBatchExtentsShaded\(", hpp)) == 2           # the context class and the pool class
    assert "std::vector<meao_target_extent>" in hpp
    body = re.search(r"\[StructLayout\(LayoutKind\.Sequential\)\]\s*public struct MeaoTargetExtent\s*\{(.*?)\}", cs, re.S)
    assert body
    cs_type = {"int32_t": "int", "uint64_t": "ulong"}
    assert re.findall(r"public (\w+) (\w+);", body.group(1)) == [(cs_type[t], n) for n, t, _ in FIELDS]


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
