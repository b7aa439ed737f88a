"""The composite into RGBA32F, RGBA8 and R11G11B10F colour targets (meao_composite_format, meao_composite_enqueue_format,
meao_pool_composite_enqueue_format): what the header leaves open, the C# wrapper, argument checks that need no device, the
tensor layouts composite_surfaces accepts under its color_format keyword, and the rule that the formats live in the kernels that
already composite: no new instantiation."""
import ctypes as C
import os

import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.surfaces import composite_surfaces
from tests import abi_model as A
from tests import kernel_inventory as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPOSITE_KERNELS = {"composite_kernel<0>", "composite_kernel<1>"} | {
    "render_with_composite_kernel<%d, %s, %d>" % (fmt, rtne, div)
    for fmt in (0, 1) for rtne, div in (("false", 0), ("false", 1), ("true", 1))}


@pytest.mark.parametrize("name", ["meao_composite_format", "meao_composite_enqueue_format", "meao_pool_composite_enqueue_format"])
def test_entry_point_in_the_header(name):
    """Where the format sits (the whole prototype, with its types and count, is pinned by tests/abi_snapshot.json)."""
    args = A.prototype(name)
    at = args.index("int32_t color_format")
    assert args[at - 1].endswith("color") and args[at + 1] == "uint64_t color_pitch"         # inserted after `color`
    for pitch in ("uint64_t ao_pitch", "uint64_t color_pitch", "uint64_t gbuffer0_pitch"):
        assert pitch in args, (name, pitch)


def test_the_header_says_what_the_formats_leave_open():
    assert "one reading" in A.header_prose().lower() and "sRGB targets are out of scope" in A.header_prose()


def test_csharp_wrapper_takes_a_colour_format():
    assert "colorFormat" in open(os.path.join(ROOT, "bindings", "csharp", "AmbientOcclusionOverMeao.cs")).read()


def test_entry_points_reject_a_null_context(meao_lib):
    ptr = (C.c_void_p * 1)(None)
    E = L.ERR_INVALID_ARGUMENT
    assert meao_lib.meao_composite_format(None, 0, None, 0, None, 1, 0, None, 0, L.MEM_DEVICE, None) == E
    assert meao_lib.meao_composite_enqueue_format(None, 0, 1, ptr, 0, ptr, 1, 0, None, 0) == E
    assert meao_lib.meao_pool_composite_enqueue_format(None, 0, 1, ptr, 0, ptr, 1, 0, None, 0) == E


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
    """A context exists only where a device does (meao_create allocates), so this one case runs with the GPU suite; every call is
    refused in validation, before anything is launched: the pointers it names are never dereferenced."""
    w = 100
    one = C.c_void_p(4096)                      # never dereferenced: every call below is refused in validation
    ptr = (C.c_void_p * 1)(4096)
    I, U = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED

    def both(fmt, ao_pitch, color_pitch, g_pitch, status, word):
        rc = meao_lib.meao_composite_format(ctx, 1, one, ao_pitch, one, fmt, color_pitch, one, g_pitch, L.MEM_DEVICE, None)
        assert rc == status, (fmt, ao_pitch, color_pitch, g_pitch)
        assert word in meao_lib.meao_last_error(ctx).decode()
        rc = meao_lib.meao_composite_enqueue_format(ctx, 1, 1, ptr, ao_pitch, ptr, fmt, color_pitch, ptr, g_pitch)
        assert rc == status, (fmt, ao_pitch, color_pitch, g_pitch)
        assert word in meao_lib.meao_last_error(ctx).decode()

    for bad in (-1, 4, 99):
        both(bad, 0, 0, 0, I, "color_format")
        both(bad, 0, w * 16, 0, I, "color_format")
    for fmt, elem in ((L.COLOR_RGBA16F, 8), (L.COLOR_RGBA32F, 16), (L.COLOR_RGBA8, 4), (L.COLOR_R11G11B10F, 4)):
        both(fmt, 0, w * elem - elem, 0, I, "color_pitch")          # smaller than a row
        both(fmt, 0, w * elem + elem // 2, 0, I, "color_pitch")     # not a multiple of the element size
        both(fmt, 0, (1 << 24) * elem, 0, U, "color_pitch")         # 2^24 texels
        both(fmt, 0, ((1 << 32) // 59 // elem + 1) * elem, 0, U, "color_pitch")      # 59 row steps pass 2^32 - 1 bytes
        both(fmt, w - 1, 0, 0, I, "ao_pitch")
        both(fmt, 0, 0, w * 4 + 2, I, "gbuffer0_pitch")
    n = C.c_int32(-1)
    assert meao_lib.meao_composite_pending(ctx, C.byref(n)) == 0 and n.value == 0


def test_composite_surfaces_accepts_each_layout_under_its_keyword_only():
    h, w = 12, 16
    ao = torch.zeros((2, h, w), dtype=torch.uint8)
    layouts = {L.COLOR_RGBA16F: torch.zeros((2, h, w, 4), dtype=torch.float16), L.COLOR_RGBA32F: torch.zeros((2, h, w, 4), dtype=torch.float32),
               L.COLOR_RGBA8: torch.zeros((2, h, w, 4), dtype=torch.uint8), L.COLOR_R11G11B10F: torch.zeros((2, h, w), dtype=torch.int32)}
    for fmt, color in layouts.items():
        a, ap, c, cp, g, gp = composite_surfaces(ao, color, None, h, w, torch.uint8, color_format=fmt)
        assert (ap, cp, g, gp) == (0, 0, None, 0) and c == [color[f].data_ptr() for f in range(2)]
        for other, wrong in layouts.items():
            if other != fmt:
                with pytest.raises(ValueError):
                    composite_surfaces(ao, wrong, None, h, w, torch.uint8, color_format=fmt)
        if fmt != L.COLOR_RGBA16F:
            with pytest.raises(ValueError):
                composite_surfaces(ao, color, None, h, w, torch.uint8)              # the default is RGBA16F, as ever
    with pytest.raises(ValueError, match="dtype"):
        composite_surfaces(ao, layouts[L.COLOR_RGBA32F], None, h, w, torch.uint8)
    with pytest.raises(ValueError, match="color_format"):
        composite_surfaces(ao, layouts[L.COLOR_RGBA8], None, h, w, torch.uint8, color_format=7)
    with pytest.raises(ValueError, match="dtype"):
        composite_surfaces(ao, torch.zeros((2, h, w), dtype=torch.float32), None, h, w, torch.uint8, color_format=L.COLOR_R11G11B10F)


def test_crops_give_pitches_in_bytes_of_the_format():
    h, w = 40, 60
    ao = torch.zeros((3, 50, 72), dtype=torch.uint8)[:, 5:5 + h, 4:4 + w]
    f32 = torch.zeros((3, 48, 66, 4), dtype=torch.float32)
    u8 = torch.zeros((3, 48, 66, 4), dtype=torch.uint8)
    packed = torch.zeros((3, 48, 66), dtype=torch.int32)
    for fmt, big, elem in ((L.COLOR_RGBA32F, f32, 16), (L.COLOR_RGBA8, u8, 4), (L.COLOR_R11G11B10F, packed, 4)):
        _, ap, c, cp, _, _ = composite_surfaces(ao, big[:, 2:2 + h, 1:1 + w], None, h, w, torch.uint8, color_format=fmt)
        assert (ap, cp) == (72, 66 * elem)
        assert c == [big.data_ptr() + ((f * 48 + 2) * 66 + 1) * elem for f in range(3)]


def test_no_new_kernel_instantiation():
    names = K.instantiations()
    assert {n for n in names if "composite" in n} == COMPOSITE_KERNELS
    assert len(names) == 359
