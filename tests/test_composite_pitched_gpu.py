"""The composite into row-pitched colour, GBuffer0 and AO surfaces (meao_composite_pitched, meao_composite_enqueue_pitched, the pool
form, composite_tensors) on the GPU.

Every surface lives inside a larger allocation whose bytes outside the width x height viewport hold 0xA5.  Expected values come
from oracle.composite run on packed copies of the viewports, with the AO of oracle.run (never the library's); after a call every
bit inside a viewport equals the oracle's (colour values the oracle gives as NaN are compared for NaN-ness only, as
tests/test_composite.py does; one probe texel per frame holds non-finite colour, so at most four channel values per frame fall
under that rule) and no byte outside one has changed -- in every way a composite can run.

Pitch kinds: "vector" (colour base and pitch multiples of 16 bytes, AO base and pitch multiples of two texels: the 16-byte form),
"scalar" (colour pitch = 8 mod 16 with the base offset by 8 bytes, an odd AO pitch: the per-texel form), "oddbase" (vector pitches,
bases that are not aligned: the per-texel form chosen by the base)."""
import ctypes as C

import numpy as np
import pytest
import torch

from miniengineao_amd import _lib as L
from tests import color_formats as CF
from tests import composite_targets
from tests import helpers as H
from tests.composite_targets import raw_of, typed
from tests.helpers import oracle_frame, ptr_array

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (131, 77), (640, 360)]      # even width; odd width (a half pair per row); more pairs per lane than the loop takes
Y0 = 2


def even(x):
    return x + (x & 1)


def odd(x):
    return x | 1


def layout(kind, w, h):
    table = {"vector": ((2, even(w + 6)), (2, even(w + 5)), (1, w + 3)), "scalar": ((1, odd(w + 4)), (1, odd(w + 4)), (3, w + 5)),
             "oddbase": ((1, even(w + 6)), (1, even(w + 5)), (2, w + 2)), "packed": ((0, w), (0, w), (0, w))}      # "packed": tight rows
    return table[kind], (0 if kind == "packed" else Y0), (h if kind == "packed" else h + Y0 + 1), 0


def halfs(raw):
    return typed(raw, CF.RGBA16F)


def is_nan(x):
    return (x & 0x7fff) > 0x7c00


class Targets(composite_targets.Targets):
    """n frames of AO (input), RGBA16F colour and RGBA8 GBuffer0 viewports at (x0, Y0) of (h + Y0 + 1)-row surfaces."""

    def __init__(self, oracle, w, h, n, ao_format, kind, seed, device="cuda"):
        rng = np.random.default_rng(seed)
        frames = [oracle_frame(oracle, w, h, ao_format, seed + f) for f in range(n)]
        self.depth = [d for d, _ in frames]
        color = [(rng.random((h, w, 4)) * 6.0).astype(np.float16).view(np.uint16) for _ in range(n)]
        for c in color:
            c[h // 3, w // 2] = [0x7c00, 0xfc00, 0x0001, 0x8000]         # the probe texel: inf, -inf, smallest subnormal, -0
        g = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
        super().__init__(w, h, CF.RGBA16F, ao_format, kind, layout(kind, w, h), [a for _, a in frames],
                         [raw_of(c, CF.RGBA16F, h, w) for c in color], g, device)

    # the pitches as they are, a packed row's included
    ao_pitch = property(lambda self: self.ao.row_bytes)
    color_pitch = property(lambda self: self.color.row_bytes)
    g_pitch = property(lambda self: self.g.row_bytes)

    def same_color(self, got, want, nan_limit, what):
        """Colour values the oracle gives as NaN are compared for NaN-ness only."""
        got, want = halfs(got), halfs(want)
        assert int(is_nan(want).sum()) <= 4, "at most the probe texel's four channels fall under the NaN rule"
        got, want = np.where(is_nan(got), 0x7e00, got), np.where(is_nan(want), 0x7e00, want)
        assert np.array_equal(got, want), (what, H.diff_report("color", got, want))

    def check(self, oracle, mode, frames=None, color=None, g=None, ao=None, untouched=()):
        """Frames `frames` (default: all) composited in `mode`, frames `untouched` as uploaded; arrays default to the device's."""
        frames = [f for f in (range(self.n) if frames is None else frames) if f not in untouched]
        super().check(mode, frames, color, g, ao)


def composite_now(ao, T, mode, stream, frames=None):
    """meao_composite_pitched, DEVICE, one call per frame, pitches as given."""
    a, c, g = T.ao_ptrs(), T.color_ptrs(), T.g_ptrs()
    for f in (range(T.n) if frames is None else frames):
        rc = ao._lib.meao_composite_pitched(ao._ctx, mode, a[f], T.ao_pitch, c[f], T.color_pitch, g[f] if mode == 1 else None,
                                            T.g_pitch, L.MEM_DEVICE, C.c_void_p(stream))
        assert rc == 0, ao._lib.meao_last_error(ao._ctx)


def enqueue(ao, T, mode, ao_pitch=None, color_pitch=None, g_pitch=None, with_g=None):
    """meao_composite_enqueue_pitched -> status; the pitches default to the surfaces' own."""
    with_g = (mode == 1) if with_g is None else with_g
    return ao._lib.meao_composite_enqueue_pitched(
        ao._ctx, mode, T.n, ptr_array(T.ao_ptrs()), T.ao_pitch if ao_pitch is None else ao_pitch,
        ptr_array(T.color_ptrs()), T.color_pitch if color_pitch is None else color_pitch,
        ptr_array(T.g_ptrs()) if with_g else None, T.g_pitch if g_pitch is None else g_pitch)


def Renders(T, n):
    return composite_targets.Renders([(T.depth[f % T.n], T.want_ao[f % T.n]) for f in range(n)], T.ao_format)


def context(oracle, T, max_batch):
    return H.component(H.settings(oracle, T.w, T.h, ao_format=T.ao_format), max_batch=max_batch)


# ---- stand-alone

@pytest.mark.parametrize("kind", ["vector", "scalar", "oddbase"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_standalone_device(oracle, mode, ao_format, w, h, kind):
    T = Targets(oracle, w, h, 2, ao_format, kind, seed=11)
    ao = context(oracle, T, 1)
    try:
        composite_now(ao, T, mode, torch.cuda.current_stream().cuda_stream)
        T.check(oracle, mode)
    finally:
        ao.close()


@pytest.mark.parametrize("kind", ["vector", "scalar"])
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_standalone_host(oracle, mode, ao_format, kind):
    T = Targets(oracle, 131, 77, 1, ao_format, kind, seed=13, device=None)
    ao = context(oracle, T, 1)
    try:
        color, g, a = T.color.host.copy(), T.g.host.copy(), T.ao.host.copy()
        rc = ao._lib.meao_composite_pitched(ao._ctx, mode, T.ao_ptrs(a.ctypes.data)[0], T.ao_pitch, T.color_ptrs(color.ctypes.data)[0],
                                            T.color_pitch, T.g_ptrs(g.ctypes.data)[0] if mode == 1 else None, T.g_pitch,
                                            L.MEM_HOST, None)
        assert rc == 0, ao._lib.meao_last_error(ao._ctx)
        T.check(oracle, mode, color=color, g=g, ao=a)
    finally:
        ao.close()


# ---- enqueued: carried by the next call's render kernel

@pytest.mark.parametrize("kind", ["vector", "scalar"])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_enqueued_and_carried(oracle, mode, ao_format, w, h, kind):
    n = 2
    T = Targets(oracle, w, h, n, ao_format, kind, seed=21)
    R = Renders(T, n)
    ao = context(oracle, T, n)
    try:
        R.execute(ao)
        assert enqueue(ao, T, mode) == 0, ao._lib.meao_last_error(ao._ctx)
        assert ao.composite_pending
        R.execute(ao)                           # carries the batch: in its texel loop for multiply, in front of the tile otherwise
        assert not ao.composite_pending
        T.check(oracle, mode)
        R.check()
    finally:
        ao.close()


def test_oddbase_batch_is_carried_in_the_scalar_form(oracle):
    T = Targets(oracle, 131, 77, 2, L.AO_R8, "oddbase", seed=23)
    R = Renders(T, 2)
    ao = context(oracle, T, 2)
    try:
        R.execute(ao)
        assert enqueue(ao, T, 0) == 0
        R.execute(ao)
        T.check(oracle, 0)
    finally:
        ao.close()


@pytest.mark.parametrize("w,h", [(1030, 40), (2601, 24), (4100, 24), (8200, 24), (32768, 32)])
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_rows_wider_than_a_workgroup_are_carried_in_chunks(oracle, ao_format, w, h):
    """A row of more than 512 pairs is 2, 4 or 8 chunks, each with a workgroup of its own (515, 1301 and 2050 pairs here; 33
    workgroups per frame at 4100 wide, so one of them owns no chunk); at 8200 wide a row is longer than the eight chunks, and at
    32768 x 32 every owning workgroup has a single row."""
    n = 2
    T = Targets(oracle, w, h, n, ao_format, "vector", seed=25)
    R = Renders(T, n)
    ao = context(oracle, T, n)
    try:
        R.execute(ao)
        assert enqueue(ao, T, 0) == 0, ao._lib.meao_last_error(ao._ctx)
        R.execute(ao)
        assert not ao.composite_pending
        T.check(oracle, 0)
        R.check()
    finally:
        ao.close()


# ---- enqueued: every other way a waiting batch runs

@pytest.mark.parametrize("kind", ["vector", "scalar"])
@pytest.mark.parametrize("mode,ao_format,w,h", [(0, L.AO_R8, 131, 77), (1, L.AO_F16, 131, 77), (0, L.AO_R8, 640, 360), (2, L.AO_R8, 64, 48)])
@pytest.mark.parametrize("way", ["flush", "second_enqueue", "other_frame_count", "per_frame_call", "resize"])
def test_waiting_batch_runs_with_its_pitches(oracle, way, mode, ao_format, w, h, kind):
    n = 2
    T = Targets(oracle, w, h, n, ao_format, kind, seed=31)
    R = Renders(T, 3)
    ao = context(oracle, T, 3)
    try:
        st = torch.cuda.current_stream().cuda_stream
        R.execute(ao, n)
        assert enqueue(ao, T, mode) == 0, ao._lib.meao_last_error(ao._ctx)
        if way == "flush":
            ao.composite_flush(st)
        elif way == "second_enqueue":
            T2 = Targets(oracle, w, h, n, ao_format, "vector" if kind == "scalar" else "scalar", seed=31)
            assert enqueue(ao, T2, mode) == 0           # pushes the first batch out, with the first batch's pitches
            assert ao.composite_pending
            T.check(oracle, mode)
            T2.check(oracle, mode, frames=())           # still waiting: untouched
            ao.composite_flush(st)
            T2.check(oracle, mode)
        elif way == "other_frame_count":
            R.execute(ao, 3)                        # three render frames, two composite frames: in front of the tiles
            R.check(3)
        elif way == "per_frame_call":
            R.execute(ao, n, params=[None] * n)     # a per-frame call carries nothing: it flushes first
            R.check(n)
        else:
            torch.cuda.synchronize()
            ao.resize(w + 8, h + 8)                     # sized for the old geometry: runs now
        assert not ao.composite_pending
        T.check(oracle, mode)
    finally:
        ao.close()


def test_exhaustive_context_flushes_first(oracle):
    w, h, n = 131, 77, 2
    T = Targets(oracle, w, h, n, L.AO_R8, "vector", seed=37)
    s = H.settings(oracle, w, h, sample_set=1)
    ao = H.component(s, max_batch=n)
    try:
        st = torch.cuda.current_stream().cuda_stream
        depth = [torch.from_numpy(d).cuda() for d in T.depth]
        out = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for _ in range(n)]
        assert enqueue(ao, T, 0) == 0
        ao.execute_device([t.data_ptr() for t in depth], [t.data_ptr() for t in out], st)
        assert not ao.composite_pending
        T.check(oracle, 0)
    finally:
        ao.close()


@pytest.mark.parametrize("kind", ["vector", "scalar"])
@pytest.mark.parametrize("mode", [0, 1])
def test_pool_of_two_members(oracle, mode, kind):
    from miniengineao_amd import AmbientOcclusionPool
    w, h, n = 131, 77, 4
    T = Targets(oracle, w, h, n, L.AO_R8, kind, seed=41)
    R = Renders(T, n)
    s = H.settings(oracle, w, h)
    pool = AmbientOcclusionPool(w, h, [0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip,
                                projection00=s.proj00, reversed_z=s.reversed_z)
    try:
        torch.cuda.synchronize()
        d, o = [t.data_ptr() for t in R.depth], [t.data_ptr() for t in R.out]
        pool.execute_device(d, o)
        pool.composite_enqueue_device(mode, T.ao_ptrs(), T.color_ptrs(), T.g_ptrs() if mode == 1 else None,
                                      ao_pitch=T.ao_pitch, color_pitch=T.color_pitch, gbuffer0_pitch=T.g_pitch)
        assert pool.composite_pending
        pool.execute_device(d, o)                       # every member carries its share
        assert not pool.composite_pending
        pool.synchronize()
        T.check(oracle, mode)
        R.check()
        T2 = Targets(oracle, w, h, n, L.AO_R8, kind, seed=41)
        pool.composite_enqueue_device(mode, T2.ao_ptrs(), T2.color_ptrs(), T2.g_ptrs() if mode == 1 else None,
                                      ao_pitch=T2.ao_pitch, color_pitch=T2.color_pitch, gbuffer0_pitch=T2.g_pitch)
        pool.composite_flush()
        pool.synchronize()
        T2.check(oracle, mode)
    finally:
        pool.close()


# ---- Python: tensors in place

@pytest.mark.parametrize("mode", [0, 1])
def test_end_to_end_crops_of_larger_targets(oracle, mode):
    """execute_tensors writes the AO into a crop of a larger uint8 surface; composite_tensors(enqueue=True) composites from that crop
    into crops of larger colour and GBuffer0 targets; the next execute carries it."""
    w, h, n = 200, 88, 2
    s = H.settings(oracle, w, h)
    frames = [oracle_frame(oracle, w, h, L.AO_R8, 50 + f) for f in range(n)]
    rng = np.random.default_rng(5)
    ao = H.component(s, max_batch=n)
    try:
        depth = torch.from_numpy(np.stack([d for d, _ in frames])).cuda()
        ao_big = torch.full((n, h + 5, w + 10), 0xA5, dtype=torch.uint8, device="cuda")
        color0 = (rng.random((n, h + 4, w + 6, 4)) * 4.0).astype(np.float16)
        g0 = rng.integers(0, 256, (n, h + 3, w + 9, 4), dtype=np.uint8)
        color_big, g_big = torch.from_numpy(color0).cuda(), torch.from_numpy(g0).cuda()
        ao_crop = ao_big[:, 3:3 + h, 4:4 + w]
        color_crop, g_crop = color_big[:, 1:1 + h, 2:2 + w, :], g_big[:, 2:2 + h, 5:5 + w, :]
        ao.execute_tensors(depth, out=ao_crop)
        ao.composite_tensors(ao_crop, color_crop, g_crop if mode == 1 else None, mode=mode, enqueue=True)
        assert ao.composite_pending
        out2 = ao.execute_tensors(depth)
        assert not ao.composite_pending
        torch.cuda.synchronize()
        want_c, want_g = color0.view(np.uint16).copy(), g0.copy()
        for f in range(n):
            assert np.array_equal(out2[f].cpu().numpy(), frames[f][1])
            assert np.array_equal(ao_crop[f].cpu().numpy(), frames[f][1])
            c = np.ascontiguousarray(want_c[f, 1:1 + h, 2:2 + w])
            g = np.ascontiguousarray(want_g[f, 2:2 + h, 5:5 + w])
            oracle.composite(frames[f][1], c, mode, L.AO_R8, g if mode == 1 else None)
            want_c[f, 1:1 + h, 2:2 + w], want_g[f, 2:2 + h, 5:5 + w] = c, g
        assert np.array_equal(color_big.cpu().numpy().view(np.uint16), want_c)          # the crops composited, the rest as it was
        assert np.array_equal(g_big.cpu().numpy(), want_g)
        # the stand-alone form of the same call, on fresh targets
        color_big2, g_big2 = torch.from_numpy(color0).cuda(), torch.from_numpy(g0).cuda()
        ao.composite_tensors(ao_crop, color_big2[:, 1:1 + h, 2:2 + w, :], g_big2[:, 2:2 + h, 5:5 + w, :] if mode == 1 else None, mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(color_big2.view(torch.int16), color_big.view(torch.int16)) and torch.equal(g_big2, g_big)
        with pytest.raises(ValueError, match=r"color\[1\]"):
            ao.composite_tensors(ao_crop, [color_crop[0], color_crop[1].cpu()])
    finally:
        ao.close()


# ---- a pitch equal to the packed row is the packed call

@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_packed_pitch_through_the_pitched_entry_points_is_the_packed_call(oracle, mode, ao_format):
    w, h, n = 131, 77, 2
    A = Targets(oracle, w, h, n, ao_format, "packed", seed=61)          # the packed entry points
    B = Targets(oracle, w, h, n, ao_format, "packed", seed=61)          # the pitched ones, pitch = the packed row
    Z = Targets(oracle, w, h, n, ao_format, "packed", seed=61)          # the pitched ones, pitch = 0
    R = Renders(A, n)
    ao = context(oracle, A, n)
    try:
        st = torch.cuda.current_stream().cuda_stream
        for f in range(n):
            ao.composite_device(mode, A.ao_ptrs()[f], A.color_ptrs()[f], A.g_ptrs()[f] if mode == 1 else 0, st)
        composite_now(ao, B, mode, st)
        torch.cuda.synchronize()
        assert torch.equal(A.color.dev, B.color.dev) and torch.equal(A.g.dev, B.g.dev)
        A.check(oracle, mode)
        # composited twice now, enqueued and carried: still the same bits
        R.execute(ao)
        ao.composite_enqueue_device(mode, A.ao_ptrs(), A.color_ptrs(), A.g_ptrs() if mode == 1 else None)
        R.execute(ao)
        assert enqueue(ao, B, mode) == 0
        R.execute(ao)
        assert enqueue(ao, Z, mode, ao_pitch=0, color_pitch=0, g_pitch=0) == 0
        R.execute(ao)
        composite_now(ao, Z, mode, st)
        torch.cuda.synchronize()
        assert torch.equal(A.color.dev, B.color.dev) and torch.equal(A.g.dev, B.g.dev)
        assert torch.equal(A.color.dev, Z.color.dev) and torch.equal(A.g.dev, Z.g.dev)
    finally:
        ao.close()


# ---- which kernels run

TRACE = r"""
import ctypes as C, torch
from miniengineao_amd import AmbientOcclusion, _lib as L
w, h, n = 640, 360, 2
ao = AmbientOcclusion(w, h, max_batch=n)
depth = torch.zeros((n, h, w), dtype=torch.float32, device="cuda") + 0.5
out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
src = torch.full((n, h, w + 16), 128, dtype=torch.uint8, device="cuda")
color = torch.ones((n, h, w + 2, 4), dtype=torch.float16, device="cuda")
torch.cuda.synchronize()
s = torch.cuda.current_stream().cuda_stream
dp, op = [depth[f].data_ptr() for f in range(n)], [out[f].data_ptr() for f in range(n)]
ao.execute_device(dp, op, stream=s)
ao.composite_tensors(src[:, :, :w], color[:, :, :w, :], enqueue=True)       # a pitched multiply batch ...
ao.execute_device(dp, op, stream=s)                                         # ... carried by a same-size shared call
torch.cuda.synchronize()
print("CARRIED_DONE")
ao.composite_tensors(src[:, :, :w], color[:, :, :w, :], enqueue=True)
ao.composite_flush(s)                                                       # n plain launches
ao.composite_tensors(src[:, :, :w], color[:, :, :w, :], enqueue=True)
ao.composite_tensors(src[:, :, :w], color[:, :, :w, :], enqueue=True)       # n more: the second enqueue pushes the first out
ao.execute_device(dp, op, stream=s, params=[None] * n)                      # n more: a per-frame call flushes first
torch.cuda.synchronize()
assert not ao.composite_pending
ao.close()
"""


def test_kernel_trace(tmp_path):
    count = H.kernel_trace(tmp_path, TRACE)
    assert "CARRIED_DONE" in count.stdout
    assert count["render_with_composite_kernel"] == 1, count
    assert count["composite_kernel"] == 3 * 2, count                     # the flush paths alone: one launch per frame
    carried = next(i for i, k in enumerate(count.short) if k.startswith("render_with_composite_kernel"))
    assert not [k for k in count.short[:carried] if k.startswith("composite_kernel")], count.short
    assert not [k for k in count.short if "pitched" in k], count.short   # packed depth and AO; the composite has no kernel of that name


# ---- validation

def test_refusals_launch_nothing_and_leave_a_waiting_batch_alone(oracle):
    from miniengineao_amd import AmbientOcclusionPool
    w, h, n = 260, 132, 1
    T = Targets(oracle, w, h, n, L.AO_F16, "vector", seed=71)           # waits throughout
    V = Targets(oracle, w, h, n, L.AO_F16, "vector", seed=71)           # what the refused calls name
    s = H.settings(oracle, w, h, ao_format=L.AO_F16)
    ao = H.component(s, max_batch=1)
    pool = AmbientOcclusionPool(w, h, [0, 0], max_batch=1, ao_format=L.AO_F16, near_clip=s.near_clip, far_clip=s.far_clip,
                                projection00=s.proj00, reversed_z=s.reversed_z)
    I, U = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED
    big = 1 << 24
    cases = [  # (ao_pitch, color_pitch, gbuffer0_pitch), status, the argument meao_last_error names
        ((w * 2 - 2, None, None), I, "ao_pitch"), ((w * 2 + 1, None, None), I, "ao_pitch"),
        ((big * 2, None, None), U, "ao_pitch"), (((big - 2) * 2, None, None), U, "ao_pitch"),            # 2^24 texels; > 2^32 - 1 bytes
        ((None, w * 8 - 8, None), I, "color_pitch"), ((None, w * 8 + 4, None), I, "color_pitch"),
        ((None, big * 8, None), U, "color_pitch"), ((None, (big - 1) * 8, None), U, "color_pitch"),
        ((None, None, w * 4 - 4), I, "gbuffer0_pitch"), ((None, None, w * 4 + 2), I, "gbuffer0_pitch"),
        ((None, None, big * 4), U, "gbuffer0_pitch"), ((None, None, (big - 1) * 4), U, "gbuffer0_pitch"),
    ]
    try:
        st = torch.cuda.current_stream().cuda_stream
        assert enqueue(ao, T, 1) == 0
        pool.composite_enqueue_device(1, T.ao_ptrs(), T.color_ptrs(), T.g_ptrs(), ao_pitch=T.ao_pitch, color_pitch=T.color_pitch,
                                      gbuffer0_pitch=T.g_pitch)
        n_pool = C.c_int32()
        for (ap, cp, gp), status, arg in cases:
            ap_, cp_, gp_ = (V.ao_pitch if ap is None else ap), (V.color_pitch if cp is None else cp), (V.g_pitch if gp is None else gp)
            assert enqueue(ao, V, 1, ap, cp, gp) == status, (ap, cp, gp)
            assert arg in ao._lib.meao_last_error(ao._ctx).decode()
            rc = ao._lib.meao_composite_pitched(ao._ctx, 1, V.ao_ptrs()[0], ap_, V.color_ptrs()[0], cp_, V.g_ptrs()[0], gp_,
                                                L.MEM_DEVICE, C.c_void_p(st))
            assert rc == status, (ap, cp, gp)
            assert arg in ao._lib.meao_last_error(ao._ctx).decode()
            rc = pool._lib.meao_pool_composite_enqueue_pitched(pool._pool, 1, 1, ptr_array(V.ao_ptrs()), ap_, ptr_array(V.color_ptrs()),
                                                               cp_, ptr_array(V.g_ptrs()), gp_)
            assert rc == status, (ap, cp, gp)
            assert ao.composite_pending and pool.composite_pending
            assert pool._lib.meao_pool_composite_pending(pool._pool, C.byref(n_pool)) == 0 and n_pool.value == 1
        torch.cuda.synchronize()
        pool.synchronize()
        V.check(oracle, 1, frames=())                   # nothing was launched on the refused calls' surfaces ...
        T.check(oracle, 1, frames=())                   # ... and the waiting batches were not run
        # gbuffer0_pitch is ignored where gbuffer0 is NULL
        assert enqueue(ao, V, 0, g_pitch=3, with_g=False) == 0          # pushes T's batch out
        T.check(oracle, 1)
        ao.composite_flush(st)
        V.check(oracle, 0)
        pool.composite_flush()
        pool.synchronize()
        torch.cuda.synchronize()
        # T was composited twice now (the context's batch, then the pool's): AMBIENT_ONLY twice
        c, g = T.expected(1, 0)
        oracle.composite(T.want_ao[0], halfs(c), 1, L.AO_F16, g)
        assert np.array_equal(T.g.texels(0), g)
    finally:
        ao.close()
        pool.close()
