"""Dynamic resolution, the part that needs no GPU: the host-plan function meao_reserve_bytes, the null-argument checks, and what
the Python and C++ wrappers offer for meao_reserve, meao_get_capacity, meao_reserve_bytes, meao_prefetch_batch_sized,
meao_pool_reserve, meao_pool_resize and meao_pool_prefetch_batch_sized (their prototypes in every mirror are
tests/test_abi_mirrors.py)."""
import ctypes as C
import inspect
import re

import pytest

from miniengineao_amd import _lib as L
from tests import abi_model as A


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
    hpp = A.read(A.HPP_PATH)
    for method in ("Reserve", "Capacity", "ReserveBytes", "PrefetchBatchSized", "Resize"):
        assert re.search(r"\b%s\(" % method, hpp), method
