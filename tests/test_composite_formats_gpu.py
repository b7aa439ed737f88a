"""The composite into RGBA32F, RGBA8 and R11G11B10F colour targets (meao_composite_format, meao_composite_enqueue_format, the pool
form, composite_tensors) on the GPU.

Expected values come from the NumPy model tests/color_formats.py applied to the AO of oracle.run (never the library's).  Every
surface lives inside a larger allocation filled with 0xA5; after a call every bit inside a viewport equals the model's and no byte
outside one has changed.  One exception: an RGBA32F channel whose model value is NaN is compared for NaN-ness only (host and
device multiply may differ in payload); the random frames hold one probe texel each with non-finite and edge values, so at most
four channel values per frame fall under it.

Layouts: "packed"; "vector" (colour base and pitch multiples of 16 bytes, AO base and pitch multiples of four texels); "scalar"
(an odd pitch in texels for colour and AO: the per-texel form for the 4-byte formats); "oddbase" (vector pitches, the colour base 4
bytes off a 16-byte boundary and the AO base one texel off).  An RGBA32F surface is vector-eligible in the "scalar" layout too (a
16-byte texel makes every pitch a multiple of 16 bytes and a lane takes one AO texel), so its per-texel form runs in "oddbase" only:
there is no pitched RGBA32F surface with an aligned base that takes the per-texel form, and so no such case here."""
import ctypes as C

import numpy as np
import pytest
import torch

from miniengineao_amd import _lib as L
from tests import color_formats as CF
from tests import composite_targets
from tests import helpers as H
from tests.composite_targets import FormatTargets as Targets
from tests.composite_targets import random_color, raw_of, typed
from tests.helpers import oracle_frame, ptr_array

pytestmark = pytest.mark.gpu

FORMATS = [CF.RGBA32F, CF.RGBA8, CF.R11G11B10F]
SHAPES = [(64, 48), (133, 77), (130, 40), (67, 33), (640, 360)]      # w mod 4 = 0, 1, 2, 3; more groups per lane than one pass
KINDS = ["packed", "vector", "scalar", "oddbase"]


def composite_now(ao, T, mode, stream, with_g=True):
    a, c, g = T.ao_ptrs(), T.color_ptrs(), T.g_ptrs()
    for f in range(T.n):
        rc = ao._lib.meao_composite_format(ao._ctx, mode, a[f], T.ao_pitch, c[f], T.fmt, T.color_pitch, g[f] if mode == 1 and with_g else None,
                                           T.g_pitch, L.MEM_DEVICE, C.c_void_p(stream))
        assert rc == 0, ao._lib.meao_last_error(ao._ctx)


def enqueue(ao, T, mode):
    return ao._lib.meao_composite_enqueue_format(ao._ctx, mode, T.n, ptr_array(T.ao_ptrs()), T.ao_pitch, ptr_array(T.color_ptrs()), T.fmt,
                                                 T.color_pitch, ptr_array(T.g_ptrs()) if mode == 1 else None, T.g_pitch)


def plain_context(w, h, ao_format, max_batch=1):
    from miniengineao_amd import AmbientOcclusion
    return AmbientOcclusion(w, h, max_batch=max_batch, ao_format=ao_format)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- exhaustive operands, R8 AO

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rgba8_every_code_times_every_r8_ao(mode):
    code, aov = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))       # texel (x, y): colour x, AO y
    T = Targets(256, 256, CF.RGBA8, L.AO_R8, "packed", [aov], [np.repeat(code[..., None], 4, axis=2)])
    ao = plain_context(256, 256, L.AO_R8)
    try:
        composite_now(ao, T, mode, stream())
        T.check(mode)
    finally:
        ao.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_r11g11b10f_every_code_times_every_r8_ao(mode):
    i = np.arange(1024 * 512, dtype=np.uint32).reshape(512, 1024)
    code, aov = i & 2047, (i >> 11).astype(np.uint8)                                              # all 2048 x 256 (R code, AO) pairs
    color = (code | (code << 11) | ((code & 1023) << 22)).astype(np.uint32)
    T = Targets(1024, 512, CF.R11G11B10F, L.AO_R8, "packed", [aov], [raw_of(color, CF.R11G11B10F, 512, 1024)])
    ao = plain_context(1024, 512, L.AO_R8)
    try:
        composite_now(ao, T, mode, stream())
        T.check(mode)
    finally:
        ao.close()


# ---- exhaustive AO, F16 storage

ALL_F16 = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)


def edge_colors(fmt):
    """16 edge values per format: 0, the smallest and largest subnormal, the smallest normal, 1, the largest finite, inf, a NaN
    code; for RGBA32F also -0, the smallest f32 subnormal and 2^-126 (times an AO below 1 it underflows gradually)."""
    if fmt == CF.RGBA32F:
        bits = [0, 1, 0x007fffff, 0x00800000, 0x3f800000, 0x7f7fffff, 0x7f800000, 0x7fc00001, 0x80000000, 0x80000001, 0x00800001,
                0x00ffffff, 0x3f7fffff, 0xbf800000, 0x3f000000, 0x40490fdb]
        return [np.array([b, bits[(k + 5) % 16], bits[(k + 9) % 16], bits[(k + 13) % 16]], np.uint32).view(np.uint8) for k, b in enumerate(bits)]
    if fmt == CF.RGBA8:
        codes = [0, 1, 2, 3, 63, 64, 127, 128, 129, 170, 191, 192, 253, 254, 255, 85]
        return [np.array([c, codes[(k + 5) % 16], codes[(k + 9) % 16], codes[(k + 13) % 16]], np.uint8) for k, c in enumerate(codes)]
    m6 = [0, 1, 0x3F, 0x40, 0x3C0, 0x7BF, 0x7C0, 0x7FF, 0x41, 0x3BF, 0x3C1, 0x400, 0x7BE, 0x7C1, 0x200, 0x1FF]
    m5 = [0, 1, 0x1F, 0x20, 0x1E0, 0x3DF, 0x3E0, 0x3FF, 0x21, 0x1DF, 0x1E1, 0x200, 0x3DE, 0x3E1, 0x100, 0x0FF]
    return [np.array([m6[k] | (m6[(k + 5) % 16] << 11) | (m5[k] << 22)], np.uint32).view(np.uint8) for k in range(16)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_f16_ao(fmt):
    """Every f16 bit pattern as AO (2 046 NaNs, infinities, negatives, subnormals): DEBUG, and MULTIPLY against 16 edge colours."""
    ao = plain_context(256, 256, L.AO_F16)
    try:
        D = Targets(256, 256, fmt, L.AO_F16, "packed", [ALL_F16], seed=3)
        composite_now(ao, D, 2, stream())
        D.check(2, nan_limit=None)
        edges = edge_colors(fmt)
        colors = [np.broadcast_to(e, (256, 256, CF.TEXEL_BYTES[fmt])).copy() for e in edges]
        M = Targets(256, 256, fmt, L.AO_F16, "packed", [ALL_F16] * 16, colors)
        composite_now(ao, M, 0, stream())
        M.check(0, nan_limit=None)
    finally:
        ao.close()


# ---- shapes x layouts x formats x modes x AO formats

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_shapes_and_layouts(oracle, ao_format, w, h, kind):
    frame = oracle_frame(oracle, w, h, ao_format, 11)[1]
    ao = plain_context(w, h, ao_format)
    try:
        for fmt in FORMATS:
            for mode, with_g in ((0, False), (1, True), (2, False)):
                T = Targets(w, h, fmt, ao_format, kind, [frame], seed=17 + fmt)
                composite_now(ao, T, mode, stream(), with_g)
                T.check(mode)
    finally:
        ao.close()


def test_ambient_only_needs_the_gbuffer0_target(oracle):
    frame = oracle_frame(oracle, 64, 48, L.AO_R8, 11)[1]
    T = Targets(64, 48, CF.RGBA8, L.AO_R8, "vector", [frame])
    ao = plain_context(64, 48, L.AO_R8)
    try:
        rc = ao._lib.meao_composite_format(ao._ctx, 1, T.ao_ptrs()[0], T.ao_pitch, T.color_ptrs()[0], T.fmt, T.color_pitch, None, 0,
                                           L.MEM_DEVICE, None)
        assert rc == L.ERR_INVALID_ARGUMENT and "GBuffer0" in ao._lib.meao_last_error(ao._ctx).decode()
        T.check(1, frames=())
    finally:
        ao.close()


# ---- every way a composite can run, n = 3 frames

W3, H3, N3 = 133, 77, 3


def Renders(oracle, w, h, ao_format, n):
    return composite_targets.Renders([oracle_frame(oracle, w, h, ao_format, 30 + f) for f in range(n)], ao_format)


@pytest.mark.parametrize("loc", ["device", "host"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_standalone(oracle, mode, fmt, loc):
    frames = [oracle_frame(oracle, W3, H3, L.AO_R8, 30 + f)[1] for f in range(N3)]
    T = Targets(W3, H3, fmt, L.AO_R8, "scalar" if loc == "host" else "vector", frames, seed=5, device=None if loc == "host" else "cuda")
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        if loc == "device":
            composite_now(ao, T, mode, stream())
            T.check(mode)
        else:
            color, g, a = T.color.host.copy(), T.g.host.copy(), T.ao.host.copy()
            for f in range(N3):
                rc = ao._lib.meao_composite_format(ao._ctx, mode, T.ao_ptrs(a.ctypes.data)[f], T.ao_pitch, T.color_ptrs(color.ctypes.data)[f],
                                                   fmt, T.color_pitch, T.g_ptrs(g.ctypes.data)[f] if mode == 1 else None, T.g_pitch,
                                                   L.MEM_HOST, None)
                assert rc == 0, ao._lib.meao_last_error(ao._ctx)
            T.check(mode, color=color, g=g, ao=a)
    finally:
        ao.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("way", ["next_execute", "flush", "second_enqueue", "resize", "per_frame_call"])
def test_enqueued_batch(oracle, way, fmt):
    mode = (0, 1, 2)[FORMATS.index(fmt)] if way in ("flush", "resize") else (1 if way == "second_enqueue" else 0)
    R = Renders(oracle, W3, H3, L.AO_R8, N3)
    T = Targets(W3, H3, fmt, L.AO_R8, "vector", R.want, seed=7)
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        R.execute(ao)
        assert enqueue(ao, T, mode) == 0, ao._lib.meao_last_error(ao._ctx)
        assert ao.composite_pending
        T.check(mode, frames=())                                # waiting: untouched
        if way == "next_execute":
            R.execute(ao)
            R.check()
        elif way == "flush":
            ao.composite_flush(stream())
        elif way == "second_enqueue":
            T2 = Targets(W3, H3, FORMATS[(FORMATS.index(fmt) + 1) % 3], L.AO_R8, "scalar", R.want, seed=8)
            assert enqueue(ao, T2, mode) == 0                   # pushes the first batch out, in the first batch's format
            assert ao.composite_pending
            T.check(mode)
            T2.check(mode, frames=())
            ao.composite_flush(stream())
            T2.check(mode)
        elif way == "resize":
            torch.cuda.synchronize()
            ao.resize(W3 + 8, H3 + 8)
        else:
            R.execute(ao, params=[None] * N3)
            R.check()
        assert not ao.composite_pending
        T.check(mode)
    finally:
        ao.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_pool_of_two_members(oracle, fmt):
    from miniengineao_amd import AmbientOcclusionPool
    R = Renders(oracle, W3, H3, L.AO_R8, N3)
    T = Targets(W3, H3, fmt, L.AO_R8, "vector", R.want, seed=9)
    s = H.settings(oracle, W3, H3)
    pool = AmbientOcclusionPool(W3, H3, [0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                                reversed_z=s.reversed_z)
    try:
        torch.cuda.synchronize()
        d, o = [t.data_ptr() for t in R.depth], [t.data_ptr() for t in R.out]
        pool.execute_device(d, o)
        pool.composite_enqueue_device(1, T.ao_ptrs(), T.color_ptrs(), T.g_ptrs(), ao_pitch=T.ao_pitch, color_pitch=T.color_pitch,
                                      gbuffer0_pitch=T.g_pitch, color_format=fmt)
        assert pool.composite_pending
        pool.execute_device(d, o)
        assert not pool.composite_pending
        pool.synchronize()
        T.check(1)
        R.check()
        T2 = Targets(W3, H3, fmt, L.AO_R8, "scalar", R.want, seed=10)
        pool.composite_enqueue_device(0, T2.ao_ptrs(), T2.color_ptrs(), None, ao_pitch=T2.ao_pitch, color_pitch=T2.color_pitch, color_format=fmt)
        pool.composite_flush()
        pool.synchronize()
        T2.check(0)
    finally:
        pool.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("enqueue_it", [False, True])
def test_composite_tensors_on_crops(oracle, enqueue_it, fmt):
    n, w, h = N3, W3, H3
    R = Renders(oracle, w, h, L.AO_R8, n)
    rng = np.random.default_rng(12)
    ao = H.component(H.settings(oracle, w, h), max_batch=n)
    try:
        ao_big = torch.full((n, h + 5, w + 10), 0xA5, dtype=torch.uint8, device="cuda")
        ao_crop = ao_big[:, 3:3 + h, 4:4 + w]
        ao.execute_tensors(torch.stack(R.depth), out=ao_crop)
        raw = np.stack([np.pad(random_color(rng, fmt, h, w), ((1, 3), (2, 4), (0, 0)), constant_values=0xA5) for _ in range(n)])
        g0 = rng.integers(0, 256, (n, h + 3, w + 9, 4), dtype=np.uint8)
        if fmt == CF.RGBA32F:
            big = torch.from_numpy(raw.view(np.float32).copy()).cuda()
        elif fmt == CF.RGBA8:
            big = torch.from_numpy(raw.copy()).cuda()
        else:
            big = torch.from_numpy(raw.view(np.int32)[..., 0].copy()).cuda()
        g_big = torch.from_numpy(g0).cuda()
        ao.composite_tensors(ao_crop, big[:, 1:1 + h, 2:2 + w], g_big[:, 2:2 + h, 5:5 + w, :], mode=1, enqueue=enqueue_it, color_format=fmt)
        if enqueue_it:
            assert ao.composite_pending
            ao.execute_tensors(torch.stack(R.depth))
            assert not ao.composite_pending
        torch.cuda.synchronize()
        got = big.cpu().numpy().view(np.uint8).reshape(raw.shape)
        want, want_g = raw.copy(), g0.copy()
        for f in range(n):
            assert np.array_equal(ao_crop[f].cpu().numpy(), R.want[f])
            c, g = CF.composite(R.want[f], L.AO_R8, typed(raw[f, 1:1 + h, 2:2 + w], fmt), fmt, 1, g0[f, 2:2 + h, 5:5 + w])
            want[f, 1:1 + h, 2:2 + w], want_g[f, 2:2 + h, 5:5 + w] = raw_of(c, fmt, h, w), g
        if fmt == CF.RGBA32F:
            nan = np.isnan(want.view(np.float32))
            assert int(nan.sum()) <= 4 * n and np.array_equal(np.isnan(got.view(np.float32)), nan)
            got.view(np.uint32)[nan], want.view(np.uint32)[nan] = 0, 0
        assert np.array_equal(got, want)
        assert np.array_equal(g_big.cpu().numpy(), want_g)
        with pytest.raises(ValueError):
            ao.composite_tensors(ao_crop, big[:, 1:1 + h, 2:2 + w])             # the default is RGBA16F, as ever
    finally:
        ao.close()


@pytest.mark.parametrize("kind", ["packed", "vector", "scalar"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rgba16f_through_the_new_entry_points_is_the_old_call(oracle, mode, kind):
    R = Renders(oracle, W3, H3, L.AO_R8, N3)
    A = Targets(W3, H3, CF.RGBA16F, L.AO_R8, kind, R.want, seed=14)
    B = Targets(W3, H3, CF.RGBA16F, L.AO_R8, kind, R.want, seed=14)
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        a, c, g = A.ao_ptrs(), A.color_ptrs(), A.g_ptrs()
        for f in range(N3):
            rc = ao._lib.meao_composite_pitched(ao._ctx, mode, a[f], A.ao_pitch, c[f], A.color_pitch, g[f] if mode == 1 else None, A.g_pitch,
                                                L.MEM_DEVICE, C.c_void_p(stream()))
            assert rc == 0
        composite_now(ao, B, mode, stream())
        torch.cuda.synchronize()
        assert torch.equal(A.color.dev, B.color.dev) and torch.equal(A.g.dev, B.g.dev)
        for f in range(N3):
            want_c, want_g = typed(A.color0[f], CF.RGBA16F).copy(), A.gbuf0[f].copy()
            oracle.composite(R.want[f], want_c, mode, L.AO_R8, want_g if mode == 1 else None)
            got = A.color.texels(f)
            assert H.nan_aware_equal(typed(got, CF.RGBA16F), want_c)[0]
            assert np.array_equal(A.g.texels(f), want_g)
        # enqueued through the new entry point, an RGBA16F batch is still carried by the render kernel (test_never_carried)
        R.execute(ao)
        assert enqueue(ao, B, mode) == 0
        R.execute(ao)
        assert not ao.composite_pending
        R.check()
    finally:
        ao.close()


# ---- which kernels run

TRACE = r"""
import ctypes as C, torch
from miniengineao_amd import AmbientOcclusion, _lib as L
w, h, n = 640, 360, 3
ao = AmbientOcclusion(w, h, max_batch=n)
depth = torch.zeros((n, h, w), dtype=torch.float32, device="cuda") + 0.5
out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
src = torch.full((n, h, w), 128, dtype=torch.uint8, device="cuda")
packed = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
half = torch.ones((n, h, w, 4), dtype=torch.float16, device="cuda")
torch.cuda.synchronize()
s = torch.cuda.current_stream().cuda_stream
dp, op = [depth[f].data_ptr() for f in range(n)], [out[f].data_ptr() for f in range(n)]
ao.execute_device(dp, op, stream=s)
ao.composite_tensors(src, packed, enqueue=True, color_format=L.COLOR_R11G11B10F)
ao.execute_device(dp, op, stream=s)                     # a shared execute: runs the R11G11B10F batch first, carries nothing
torch.cuda.synchronize()
assert not ao.composite_pending
print("PLAIN_DONE")
ao.composite_tensors(src, half, enqueue=True, color_format=L.COLOR_RGBA16F)
ao.execute_device(dp, op, stream=s)                     # an RGBA16F batch is carried as ever
torch.cuda.synchronize()
assert not ao.composite_pending
ao.close()
"""


def test_never_carried(tmp_path):
    count = H.kernel_trace(tmp_path, TRACE)
    assert "PLAIN_DONE" in count.stdout
    assert count["composite_kernel"] == 3, count                            # once per frame of the R11G11B10F batch
    assert all(k == "composite_kernel<0>" for k in count.short if k.startswith("composite_kernel")), count.short
    assert count["render_with_composite_kernel"] == 1, count                # the RGBA16F batch alone
    # the shared render kernels that carry nothing (which one a 640 x 360 batch takes is the planner's choice)
    renders = [i for i, k in enumerate(count.short) if k.split("<")[0] in ("render_kernel", "render_small_kernel", "render_wide_kernel")]
    assert len(renders) == 2, count.short                                   # the first two executes; the third is the carrying kernel
    plain = [i for i, k in enumerate(count.short) if k.startswith("composite_kernel")]
    carried = next(i for i, k in enumerate(count.short) if k.startswith("render_with_composite_kernel"))
    assert renders[0] < plain[0] and any(plain[-1] < i < carried for i in renders), count.short        # in front of that execute's passes


def test_selftest_small_float_stores():
    ao = plain_context(64, 48, L.AO_R8)
    try:
        assert ao.selftest(8) == 0
    finally:
        ao.close()
