"""The composite into sRGB colour targets (MEAO_COLOR_RGBA8_SRGB) on the GPU, through every entry point that takes a color_format.

Expected values come from the NumPy model tests/srgb_format.py (its tables computed with mpmath, not read from the library's
include) applied to the oracle's AO or to exhaustive operand frames, and are compared bit for bit.  Surfaces are the guarded
Targets of tests/composite_targets.py in the layouts of tests/test_composite_formats_gpu.py ("packed", "vector", "scalar",
"oddbase"): every byte outside a viewport must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.ambient_occlusion import target_extents_array
from tests import color_formats as CF
from tests import composite_targets
from tests import helpers as H
from tests import mixed_size as M
from tests import srgb_format as S
from tests.composite_targets import FormatTargets
from tests.helpers import oracle_frame, ptr_array

pytestmark = pytest.mark.gpu

SRGB = L.COLOR_RGBA8_SRGB
SHAPES = [(64, 48), (133, 77), (130, 40), (67, 33), (640, 360)]      # w mod 4 = 0, 1, 2, 3; more groups per lane than one pass
KINDS = ["packed", "vector", "scalar", "oddbase"]
MODES = ((0, False), (1, True), (2, False))


class Targets(FormatTargets):
    """FormatTargets with the RGBA8 layout (4-byte texels of uint8 channels) whose expectations come from tests/srgb_format.py."""

    def __init__(self, w, h, ao_format, kind, ao_frames, color_frames=None, seed=1, device="cuda"):
        super().__init__(w, h, CF.RGBA8, ao_format, kind, ao_frames, color_frames, seed, device)
        self.fmt = SRGB

    def expected(self, mode, f, with_g=True):
        g0 = self.gbuf0[f] if mode == 1 and with_g else None
        c, g = S.composite(self.want_ao[f], self.ao_format, self.color0[f], SRGB, mode, g0)
        return c, (g if g is not None else self.gbuf0[f])


def stream():
    return torch.cuda.current_stream().cuda_stream


def err(ao):
    return ao._lib.meao_last_error(ao._ctx).decode()


def plain_context(w, h, ao_format, max_batch=1):
    from miniengineao_amd import AmbientOcclusion
    return AmbientOcclusion(w, h, max_batch=max_batch, ao_format=ao_format)


def composite_now(ao, T, mode, with_g=True, loc=L.MEM_DEVICE, bases=(None, None, None)):
    a, c, g = T.ao_ptrs(bases[0]), T.color_ptrs(bases[1]), T.g_ptrs(bases[2])
    for f in range(T.n):
        rc = ao._lib.meao_composite_format(ao._ctx, mode, a[f], T.ao_pitch, c[f], SRGB, T.color_pitch, g[f] if mode == 1 and with_g else None,
                                           T.g_pitch, loc, C.c_void_p(stream()) if loc == L.MEM_DEVICE else None)
        assert rc == 0, err(ao)


# ---- exhaustive operands

@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_code_times_every_r8_ao(mode):
    code, aov = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))       # texel (x, y): colour x, AO y
    color = np.stack([code, code, code[:, ::-1], code], axis=-1)                                     # b runs the other way
    T = Targets(256, 256, L.AO_R8, "packed", [aov], [color])
    ao = plain_context(256, 256, L.AO_R8)
    try:
        composite_now(ao, T, mode)
        T.check(mode)
    finally:
        ao.close()


ALL_F16 = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
EDGES = [0, 1, 10, 11, 127, 128, 254, 255]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_f16_ao_against_edge_colours(mode):
    """Every f16 bit pattern as AO: NaNs of both signs, infinities, negatives, subnormals and factors above 1."""
    colors = [np.broadcast_to(np.array([e, EDGES[(k + 3) % 8], EDGES[(k + 5) % 8], e], np.uint8), (256, 256, 4)).copy() for k, e in enumerate(EDGES)]
    T = Targets(256, 256, L.AO_F16, "packed", [ALL_F16] * len(EDGES), colors)
    ao = plain_context(256, 256, L.AO_F16)
    try:
        composite_now(ao, T, mode)
        T.check(mode)
    finally:
        ao.close()


# ---- shapes x layouts x modes x AO formats

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_shapes_and_layouts(oracle, ao_format, w, h, kind):
    frame = oracle_frame(oracle, w, h, ao_format, 11)[1]
    ao = plain_context(w, h, ao_format)
    try:
        for mode, with_g in MODES:
            T = Targets(w, h, ao_format, kind, [frame], seed=17 + mode)
            composite_now(ao, T, mode, with_g)
            T.check(mode)
    finally:
        ao.close()


# ---- one case per entry point

W3, H3, N3 = 133, 77, 3


def renders(oracle, n=N3):
    return composite_targets.Renders([oracle_frame(oracle, W3, H3, L.AO_R8, 30 + f) for f in range(n)], L.AO_R8)


@pytest.mark.parametrize("loc", ["device", "host"])
def test_standalone(oracle, loc):
    frames = [oracle_frame(oracle, W3, H3, L.AO_R8, 30 + f)[1] for f in range(N3)]
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        for mode, _ in MODES:
            if loc == "device":
                T = Targets(W3, H3, L.AO_R8, "vector", frames, seed=5)
                composite_now(ao, T, mode)
                T.check(mode)
            else:
                T = Targets(W3, H3, L.AO_R8, "scalar", frames, seed=5, device=None)
                color, g, a = T.color.host.copy(), T.g.host.copy(), T.ao.host.copy()
                composite_now(ao, T, mode, loc=L.MEM_HOST, bases=(a.ctypes.data, color.ctypes.data, g.ctypes.data))
                T.check(mode, color=color, g=g, ao=a)
    finally:
        ao.close()


@pytest.mark.parametrize("way", ["next_execute", "flush", "per_frame_call"])
def test_enqueued_batch(oracle, way):
    mode = {"next_execute": 0, "flush": 1, "per_frame_call": 2}[way]
    R = renders(oracle)
    T = Targets(W3, H3, L.AO_R8, "vector", R.want, seed=7)
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        R.execute(ao)
        rc = ao._lib.meao_composite_enqueue_format(ao._ctx, mode, T.n, ptr_array(T.ao_ptrs()), T.ao_pitch, ptr_array(T.color_ptrs()), SRGB,
                                                   T.color_pitch, ptr_array(T.g_ptrs()) if mode == 1 else None, T.g_pitch)
        assert rc == 0, err(ao)
        assert ao.composite_pending
        T.check(mode, frames=())                                # waiting: untouched
        if way == "next_execute":
            R.execute(ao)                                       # never carried: this execute runs the batch first
            R.check()
        elif way == "flush":
            ao.composite_flush(stream())
        else:
            R.execute(ao, params=[None] * N3)
            R.check()
        assert not ao.composite_pending
        T.check(mode)
    finally:
        ao.close()


def test_composite_batch_of_three_frames(oracle):
    frames = [oracle_frame(oracle, W3, H3, L.AO_R8, 30 + f)[1] for f in range(N3)]
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        for (mode, with_g), kind in zip(MODES, ("vector", "oddbase", "packed")):
            T = Targets(W3, H3, L.AO_R8, kind, frames, seed=40 + mode)
            rc = ao._lib.meao_composite_batch(ao._ctx, mode, N3, ptr_array(T.ao_ptrs()), T.ao_pitch, ptr_array(T.color_ptrs()), SRGB, T.color_pitch,
                                              ptr_array(T.g_ptrs()) if with_g else None, T.g_pitch, C.c_void_p(stream()))
            assert rc == 0, err(ao)
            assert not ao.composite_pending
            T.check(mode)
    finally:
        ao.close()


def shaded_targets(R, kind, seed):
    """Targets whose AO pointers are the execute's outputs (the Targets' own AO surface stays an unused input)."""
    T = Targets(W3, H3, L.AO_R8, kind, R.want, seed=seed)
    T.ao_ptrs = lambda base=None: [t.data_ptr() for t in R.out]
    return T


def test_execute_batch_shaded(oracle):
    R = renders(oracle)
    ao = H.component(H.settings(oracle, W3, H3), max_batch=N3)
    try:
        for (mode, with_g), kind in zip(MODES, ("vector", "oddbase", "packed")):
            T = shaded_targets(R, kind, 50 + mode)
            for t in R.out:
                t.fill_(0xA5)
            ao.execute_shaded_device([t.data_ptr() for t in R.depth], T.ao_ptrs(), mode, T.color_ptrs(), T.g_ptrs() if with_g else None, stream(),
                                     color_pitch=T.color_pitch, gbuffer0_pitch=T.g_pitch, color_format=SRGB)
            assert not ao.composite_pending
            R.check()
            T.check(mode, ao=T.ao.host)
    finally:
        ao.close()


SIZES = M.ORDER[:1] + M.ORDER[2:]                   # (33, 17), (200, 120), (97, 61): frames of the mixed-size suites, their AO cached
SIZED_KINDS = ("vector", "oddbase", "packed")       # the second frame is not vector-eligible: each frame keeps its own form


def test_composite_batch_extents(oracle):
    base = M.base_settings(oracle)
    call = M.MixedCall(torch, oracle, base, SIZES)
    Ts = [Targets(w, h, L.AO_R8, SIZED_KINDS[f], [call.want(f)["result"]], seed=60 + f) for f, (w, h) in enumerate(SIZES)]
    ao = M.context(base)
    try:
        ext = [(T.w, T.h, T.ao_pitch, T.color_pitch, T.g_pitch) for T in Ts]
        rc = ao._lib.meao_composite_batch_extents(ao._ctx, 1, len(Ts), ptr_array([T.ao_ptrs()[0] for T in Ts]),
                                                  ptr_array([T.color_ptrs()[0] for T in Ts]), SRGB, ptr_array([T.g_ptrs()[0] for T in Ts]),
                                                  target_extents_array(ext, len(Ts)), C.c_void_p(stream()))
        assert rc == 0, err(ao)
        for T in Ts:
            T.check(1)
    finally:
        ao.close()


def test_execute_batch_extents_shaded(oracle):
    base = M.base_settings(oracle)
    call = M.MixedCall(torch, oracle, base, SIZES)
    Ts = [Targets(w, h, L.AO_R8, SIZED_KINDS[f], [call.want(f)["result"]], seed=70 + f) for f, (w, h) in enumerate(SIZES)]
    ao = M.context(base)
    try:
        ao.execute_shaded_device([d.ptr for d in call.depth], [o.ptr for o in call.out], 0, [T.color_ptrs()[0] for T in Ts], None,
                                 params=call.params, color_format=SRGB, extents=call.extents, color_pitches=[T.color_pitch for T in Ts],
                                 gbuffer0_pitches=[T.g_pitch for T in Ts])
        assert not ao.composite_pending
        call.check(ao, debug_buffers=False)
        for T in Ts:
            T.check(0, ao=T.ao.host)
    finally:
        ao.close()


def test_pool_of_two_members(oracle):
    from miniengineao_amd import AmbientOcclusionPool
    R = renders(oracle)
    T = shaded_targets(R, "vector", 80)
    s = H.settings(oracle, W3, H3)
    pool = AmbientOcclusionPool(W3, H3, [0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                                reversed_z=s.reversed_z)
    try:
        torch.cuda.synchronize()
        pool.execute_shaded_device([t.data_ptr() for t in R.depth], T.ao_ptrs(), 1, T.color_ptrs(), T.g_ptrs(), color_pitch=T.color_pitch,
                                   gbuffer0_pitch=T.g_pitch, color_format=SRGB)
        assert not pool.composite_pending
        pool.synchronize()
        R.check()
        T.check(1, ao=T.ao.host)
    finally:
        pool.close()


def test_ambient_only_leaves_gbuffer0_as_rgba8_does(oracle):
    frame = oracle_frame(oracle, W3, H3, L.AO_R8, 30)[1]
    A = Targets(W3, H3, L.AO_R8, "vector", [frame], seed=90)
    B = FormatTargets(W3, H3, CF.RGBA8, L.AO_R8, "vector", [frame], seed=90)       # the same colour and GBuffer0 bytes
    ao = plain_context(W3, H3, L.AO_R8)
    try:
        composite_now(ao, A, 1)
        a, c, g = B.ao_ptrs(), B.color_ptrs(), B.g_ptrs()
        rc = ao._lib.meao_composite_format(ao._ctx, 1, a[0], B.ao_pitch, c[0], CF.RGBA8, B.color_pitch, g[0], B.g_pitch, L.MEM_DEVICE,
                                           C.c_void_p(stream()))
        assert rc == 0, err(ao)
        A.check(1)
        B.check(1)
        assert torch.equal(A.g.dev, B.g.dev)
        assert not torch.equal(A.color.dev, B.color.dev)        # and the colours differ: linear light against stored codes
    finally:
        ao.close()


def test_selftest_srgb_conversions():
    ao = plain_context(64, 48, L.AO_R8)
    try:
        assert ao.selftest(9) == 0
    finally:
        ao.close()
