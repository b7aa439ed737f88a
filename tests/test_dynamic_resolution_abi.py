"""Dynamic resolution, the part that needs no GPU: the prototypes in include/meao.h, the host-plan function meao_reserve_bytes, and
the Python, C++ and C# mirrors of the new calls (meao_reserve, meao_get_capacity, meao_reserve_bytes, meao_prefetch_batch_sized,
meao_pool_reserve, meao_pool_resize, meao_pool_prefetch_batch_sized)."""
import ctypes as C
import inspect
import os
import re

import pytest

from miniengineao_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "meao.h")).read()
NEW_CALLS = {"meao_reserve": 3, "meao_get_capacity": 3, "meao_reserve_bytes": 4, "meao_prefetch_batch_sized": 7,
             "meao_pool_reserve": 3, "meao_pool_resize": 3, "meao_pool_prefetch_batch_sized": 7}


def config(meao_lib, **fields):
    cfg = L.Config()
    meao_lib.meao_default_config(C.byref(cfg))
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def reserve_bytes(meao_lib, cfg, w, h):
    b = C.c_uint64()
    assert meao_lib.meao_reserve_bytes(C.byref(cfg), w, h, C.byref(b)) == L.OK, (w, h)
    return b.value


def level_px(meao_lib, w, h, k):
    lw, lh = C.c_int32(), C.c_int32()
    assert meao_lib.meao_level_dims(w, h, k, C.byref(lw), C.byref(lh)) == L.OK
    return lw.value * lh.value


def test_header_carries_the_prototypes_and_the_abi_version_stays():
    for name, nargs in NEW_CALLS.items():
        m = re.search(r"MEAO_API\s+int32_t\s+%s\s*\((.*?)\);" % name, HEADER, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    assert re.search(r"#define\s+MEAO_ABI_VERSION\s+7\b", HEADER)
    assert L.ABI_VERSION == 7
    assert "meao_test_counters" not in HEADER          # the test hook is no part of the product's interface


def test_library_exports_the_calls(meao_lib):
    for name in NEW_CALLS:
        assert name in L.SIGNATURES and getattr(meao_lib, name)
    assert meao_lib.meao_abi_version() == 7
    assert not hasattr(meao_lib, "meao_test_counters")


@pytest.mark.parametrize("fields", [dict(), dict(ao_format=L.AO_F16, hq_levels=2, max_batch=3), dict(num_levels=2, pipelined=1)])
def test_reserve_bytes_is_monotone_in_each_dimension(meao_lib, fields):
    cfg = config(meao_lib, **fields)
    # every width / height step across two whole periods of the coarsest level (16 texels) and some large ones
    sizes = list(range(1, 40)) + [97, 200, 380, 384, 400, 1920, 3840, 32768]
    for fixed in (1, 17, 272, 2160):
        by_w = [reserve_bytes(meao_lib, cfg, w, fixed) for w in sizes]
        by_h = [reserve_bytes(meao_lib, cfg, fixed, h) for h in sizes]
        assert by_w == sorted(by_w) and by_h == sorted(by_h), fixed
    assert reserve_bytes(meao_lib, cfg, 400, 272) > reserve_bytes(meao_lib, cfg, 384, 256) > 0


@pytest.mark.parametrize("w,h", [(400, 272), (33, 17), (3840, 2160), (1, 1)])
def test_pipelined_costs_exactly_one_more_downsample_set_per_slot(meao_lib, w, h):
    # a downsample set: LowDepth1..4 in f32, each buffer aligned to 256 bytes
    ds_set = sum((level_px(meao_lib, w, h, k) * 4 + 255) // 256 * 256 for k in range(1, 5))
    for batch in (1, 2, 5):
        one = reserve_bytes(meao_lib, config(meao_lib, max_batch=batch, pipelined=0), w, h)
        two = reserve_bytes(meao_lib, config(meao_lib, max_batch=batch, pipelined=1), w, h)
        assert two - one == batch * ds_set, (batch, one, two)


@pytest.mark.parametrize("pipelined", [0, 1])
def test_reserve_bytes_is_max_batch_times_one_slot(meao_lib, pipelined):
    one = reserve_bytes(meao_lib, config(meao_lib, max_batch=1, pipelined=pipelined, ao_format=L.AO_F16), 400, 272)
    for batch in (2, 7, 64):
        assert reserve_bytes(meao_lib, config(meao_lib, max_batch=batch, pipelined=pipelined, ao_format=L.AO_F16), 400, 272) == batch * one


def test_reserve_bytes_needs_no_current_size(meao_lib):
    """Host-plan only: the figure is that of the reserved size, whatever size the configuration names."""
    a = reserve_bytes(meao_lib, config(meao_lib, width=8, height=8), 400, 272)
    assert a == reserve_bytes(meao_lib, config(meao_lib, width=3840, height=2160), 400, 272)


def test_reserve_bytes_rejects_sizes_outside_the_range(meao_lib):
    cfg = config(meao_lib)
    b = C.c_uint64()
    for w, h in ((0, 10), (10, 0), (-1, 10), (10, -1), (32769, 10), (10, 32769), (0, 0)):
        assert meao_lib.meao_reserve_bytes(C.byref(cfg), w, h, C.byref(b)) == L.ERR_INVALID_ARGUMENT, (w, h)
    assert meao_lib.meao_reserve_bytes(C.byref(cfg), 32768, 32768, C.byref(b)) == L.OK
    assert meao_lib.meao_reserve_bytes(C.byref(cfg), 1, 1, C.byref(b)) == L.OK
    assert meao_lib.meao_reserve_bytes(None, 10, 10, C.byref(b)) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_reserve_bytes(C.byref(cfg), 10, 10, None) == L.ERR_INVALID_ARGUMENT
    bad = config(meao_lib, num_levels=9)
    assert meao_lib.meao_reserve_bytes(C.byref(bad), 10, 10, C.byref(b)) == L.ERR_INVALID_ARGUMENT


def test_null_contexts_are_refused(meao_lib):
    w, h = C.c_int32(), C.c_int32()
    assert meao_lib.meao_reserve(None, 10, 10) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_get_capacity(None, C.byref(w), C.byref(h)) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_prefetch_batch_sized(None, 8, 8, 1, (C.c_void_p * 1)(1), 0, None) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_reserve(None, 10, 10) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_resize(None, 10, 10) == L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_pool_prefetch_batch_sized(None, 8, 8, 1, (C.c_void_p * 1)(1), 0, None) == L.ERR_INVALID_ARGUMENT


def test_python_signatures():
    from miniengineao_amd import AmbientOcclusion, AmbientOcclusionPool
    for cls in (AmbientOcclusion, AmbientOcclusionPool):
        size = inspect.signature(cls.prefetch_device).parameters["size"]
        assert size.kind is inspect.Parameter.KEYWORD_ONLY and size.default is None, cls
        assert list(inspect.signature(cls.reserve).parameters) == ["self", "max_width", "max_height"], cls
        assert list(inspect.signature(cls.resize).parameters) == ["self", "width", "height"], cls
    assert isinstance(AmbientOcclusion.capacity, property)


def test_cpp_and_csharp_mirrors_carry_the_calls():
    hpp = open(os.path.join(ROOT, "include", "meao.hpp")).read()
    cs = open(os.path.join(ROOT, "bindings", "csharp", "MeaoNative.cs")).read()
    for name in NEW_CALLS:
        assert re.search(r"\b%s\(" % name, hpp), name
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, cs), name
    for method in ("Reserve", "Capacity", "ReserveBytes", "PrefetchBatchSized", "Resize"):
        assert re.search(r"\b%s\(" % method, hpp), method
