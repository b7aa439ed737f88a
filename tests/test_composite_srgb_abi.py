"""MEAO_COLOR_RGBA8_SRGB: its texel size and host layout in Python, its name in the C++ wrapper, the definition the header gives
(its value in every binding is tests/test_abi_mirrors.py), the tensor layout composite_surfaces accepts under color_format=5,
the refusals that need no launch, and the rule that the format lives in the kernels that already composite."""
import ctypes as C

import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.surfaces import color_layout, composite_surfaces
from tests import abi_model as A
from tests import kernel_inventory as K
from tests.test_composite_formats_abi import COMPOSITE_KERNELS


def test_the_enum_in_every_binding():
    assert 4 not in A.header_model()["enums"]["meao_color_format"].values()                 # 4 stays unassigned
    assert L.COLOR_TEXEL_BYTES[L.COLOR_RGBA8_SRGB] == 4 and set(L.COLOR_TEXEL_BYTES) == set(A.header_model()["enums"]["meao_color_format"].values())
    assert "RGBA8_SRGB" in A.read(A.HPP_PATH)
    from miniengineao_amd.ambient_occlusion import AmbientOcclusion
    assert AmbientOcclusion._HOST_COLOR[L.COLOR_RGBA8_SRGB] == AmbientOcclusion._HOST_COLOR[L.COLOR_RGBA8]


def test_the_header_defines_the_format_and_the_selftest():
    for word in ("0x399f22b4", "0x3f7edc0e", "48a8f05136456237aae2c5349e5f0199a182daa19b7c099eb542058f794b9c5b",
                 "0b408a80ff623c35aef23dc30ed2669cc9893ecc3227e21394a963f4e5bb51de",
                 "c7ccee49d6fa41ef4c5a950ae2d9263efd487244dee3eeef6adbc3091ffb79df", "0.04045", "12.92"):
        assert word in A.header_text(), word
    assert " 9 = the conversions of MEAO_COLOR_RGBA8_SRGB" in A.header_prose()


def test_composite_surfaces_accepts_the_uint8_layout_only():
    h, w = 12, 16
    ao = torch.zeros((2, h, w), dtype=torch.uint8)
    assert color_layout(L.COLOR_RGBA8_SRGB) == color_layout(L.COLOR_RGBA8)
    color = torch.zeros((2, h, w, 4), dtype=torch.uint8)
    a, ap, c, cp, g, gp = composite_surfaces(ao, color, None, h, w, torch.uint8, color_format=L.COLOR_RGBA8_SRGB)
    assert (ap, cp, g, gp) == (0, 0, None, 0) and c == [color[f].data_ptr() for f in range(2)]
    crop = torch.zeros((2, h + 3, w + 5, 4), dtype=torch.uint8)[:, 1:1 + h, 2:2 + w]
    assert composite_surfaces(ao, crop, None, h, w, torch.uint8, color_format=L.COLOR_RGBA8_SRGB)[3] == (w + 5) * 4
    for wrong in (torch.zeros((2, h, w, 4), dtype=torch.float16), torch.zeros((2, h, w, 4), dtype=torch.float32),
                  torch.zeros((2, h, w), dtype=torch.int32), torch.zeros((2, h, w, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            composite_surfaces(ao, wrong, None, h, w, torch.uint8, color_format=L.COLOR_RGBA8_SRGB)
    with pytest.raises(ValueError, match="color_format"):
        composite_surfaces(ao, color, None, h, w, torch.uint8, color_format=4)


@pytest.fixture()
def ctx(meao_lib):
    cfg = L.Config()
    meao_lib.meao_default_config(C.byref(cfg))
    cfg.width, cfg.height, cfg.max_batch = 100, 60, 2
    handle = C.c_void_p()
    assert meao_lib.meao_create(C.byref(cfg), C.byref(handle)) == 0
    yield handle
    meao_lib.meao_destroy(handle)


@pytest.mark.gpu
def test_refusals_launch_nothing(meao_lib, ctx):
    """As tests/test_composite_formats_abi.py: a context exists only where a device does; every call is refused in validation,
    before anything is launched, and the pointers it names are never dereferenced."""
    w, fmt, elem = 100, L.COLOR_RGBA8_SRGB, 4
    one = C.c_void_p(4096)
    ptr = (C.c_void_p * 1)(4096)
    I, U = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED

    def both(fmt, ao_pitch, color_pitch, g_pitch, status, word):
        rc = meao_lib.meao_composite_format(ctx, 1, one, ao_pitch, one, fmt, color_pitch, one, g_pitch, L.MEM_DEVICE, None)
        assert rc == status, (fmt, ao_pitch, color_pitch, g_pitch)
        assert word in meao_lib.meao_last_error(ctx).decode()
        rc = meao_lib.meao_composite_enqueue_format(ctx, 1, 1, ptr, ao_pitch, ptr, fmt, color_pitch, ptr, g_pitch)
        assert rc == status, (fmt, ao_pitch, color_pitch, g_pitch)
        assert word in meao_lib.meao_last_error(ctx).decode()
        rc = meao_lib.meao_composite_batch(ctx, 1, 1, ptr, ao_pitch, ptr, fmt, color_pitch, ptr, g_pitch, None)
        assert rc == status, (fmt, ao_pitch, color_pitch, g_pitch)
        assert word in meao_lib.meao_last_error(ctx).decode()

    both(4, 0, 0, 0, I, "color_format")
    both(4, 0, w * 4, 0, I, "color_format")
    both(6, 0, 0, 0, I, "color_format")
    both(fmt, 0, w * elem - elem, 0, I, "color_pitch")          # smaller than a row
    both(fmt, 0, w * elem + elem // 2, 0, I, "color_pitch")     # not a multiple of the element size
    both(fmt, 0, (1 << 24) * elem, 0, U, "color_pitch")         # 2^24 texels
    both(fmt, 0, ((1 << 32) // 59 // elem + 1) * elem, 0, U, "color_pitch")      # 59 row steps pass 2^32 - 1 bytes
    both(fmt, w - 1, 0, 0, I, "ao_pitch")
    both(fmt, 0, 0, w * 4 + 2, I, "gbuffer0_pitch")
    n = C.c_int32(-1)
    assert meao_lib.meao_composite_pending(ctx, C.byref(n)) == 0 and n.value == 0
    bad = C.c_uint64(0)
    assert meao_lib.meao_selftest(ctx, 10, C.byref(bad)) == I


def test_no_new_kernel_instantiation():
    names = K.instantiations()
    assert {n for n in names if "composite" in n} == COMPOSITE_KERNELS
    assert len(names) == 359
