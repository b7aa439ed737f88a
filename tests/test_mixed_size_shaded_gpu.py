"""Shaded frames from mixed-size batches on the GPU: meao_composite_batch_extents (the batched composite with one size and one set of
pitches per frame), meao_execute_batch_extents_shaded, the pool form and the tensor forms.

A context of 400 x 272, max_batch 8 unless a test says otherwise.  Expected colours never come from the library: RGBA16F from
oracle.composite, the other formats from the NumPy model tests/color_formats.py, both applied to the oracle's AO of the frame at its
own size (random AO codes where a shape is too small for the oracle or the AO's content is beside the point: the composite takes
any AO surface).  Every frame has one tests/composite_targets.FormatTargets of its own: viewports inside 0xA5-filled allocations
whose other bytes must come back untouched.  The execute half of the shaded calls is a tests/mixed_size.MixedCall."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd.ambient_occlusion import target_extents_array
from tests import color_formats as CF
from tests import helpers as H
from tests import mixed_size as M
from tests.composite_targets import Y0, FormatTargets, Targets, random_color
from tests.helpers import colour, oracle_frame, ptr_array
from tests.mixed_size import CTX, MAX_BATCH, ORDER, MixedCall, base_settings, context

pytestmark = pytest.mark.gpu

ALL_FORMATS = [CF.RGBA16F, CF.RGBA32F, CF.RGBA8, CF.R11G11B10F]
MODES = ((0, False), (1, True), (2, False))
KINDS = ("packed", "vector", "oddbase")
SIZES = [(33, 17), (97, 61), (400, 272), (66, 50), (67, 49)]


def err(ao):
    return ao._lib.meao_last_error(ao._ctx).decode()


def pending(ao):
    n = C.c_int32(-1)
    assert ao._lib.meao_composite_pending(ao._ctx, C.byref(n)) == 0
    return n.value


def random_ao(rng, w, h, ao_format):
    if ao_format == L.AO_R8:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    return rng.random((h, w)).astype(np.float16).view(np.uint16)


def ao_of(oracle, w, h, ao_format, seed):
    """The oracle's AO of a synthetic frame at its own size; random codes for shapes below one tile of the coarsest level."""
    if w >= 16 and h >= 16:
        return oracle_frame(oracle, w, h, ao_format, seed)[1]
    return random_ao(np.random.default_rng(seed), w, h, ao_format)


class Sized:
    """The frames of one sized call: Ts[f] holds frame f alone (n = 1), so every frame has its own size, layout and allocations."""

    def __init__(self, Ts):
        self.Ts, self.n, self.fmt = list(Ts), len(Ts), Ts[0].fmt

    @classmethod
    def of(cls, sizes, fmt, ao_format, aos, seed, kinds=KINDS, shift=0):
        return cls([FormatTargets(w, h, fmt, ao_format, kinds[(f + shift) % len(kinds)], [aos[f]], seed=seed + f)
                    for f, (w, h) in enumerate(sizes)])

    def extents(self):
        return [(T.w, T.h, T.ao_pitch, T.color_pitch, T.g_pitch) for T in self.Ts]

    def ao_ptrs(self):
        return [T.ao_ptrs()[0] for T in self.Ts]

    def color_ptrs(self):
        return [T.color_ptrs()[0] for T in self.Ts]

    def g_ptrs(self):
        return [T.g_ptrs()[0] for T in self.Ts]

    def call(self, ao, mode, with_g=True, n=None, extents=None, aos=None, colors=None, fmt=None, stream=0):
        n = self.n if n is None else n
        k = max(n, self.n)
        pad = lambda p: ptr_array(list(p) + [p[0]] * (k - len(p)))
        ext = list(self.extents() if extents is None else extents)
        ext += [ext[0]] * (k - len(ext))
        return ao._lib.meao_composite_batch_extents(ao._ctx, mode, n, pad(self.ao_ptrs() if aos is None else aos),
                                                    pad(self.color_ptrs() if colors is None else colors), self.fmt if fmt is None else fmt,
                                                    pad(self.g_ptrs()) if mode == 1 and with_g else None, target_extents_array(ext, k),
                                                    C.c_void_p(stream) if stream else None)

    def check(self, mode, frames=None, ao_is_input=True, what=""):
        for f, T in enumerate(self.Ts):
            try:
                T.check(mode, frames=(0,) if frames is None or f in frames else (), ao=None if ao_is_input else T.ao.host)
            except AssertionError as e:
                raise AssertionError(f"{what} frame {f} ({T.w} x {T.h}, {T.kind}): {e}") from e


def big_context(oracle, ao_format=L.AO_R8, **kw):
    return H.component(H.settings(oracle, *CTX, ao_format=ao_format), max_batch=MAX_BATCH, **kw)


# ---- sizes x layouts x formats x modes x AO formats

@pytest.mark.parametrize("order", ["given", "reversed"])
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_sizes_layouts_formats_modes(oracle, ao_format, order):
    sizes = SIZES if order == "given" else SIZES[::-1]
    aos = [ao_of(oracle, w, h, ao_format, 40 + w) for w, h in sizes]
    ao = big_context(oracle, ao_format)
    ref = big_context(oracle, ao_format)
    try:
        ref.reserve(*CTX)
        for k, fmt in enumerate(ALL_FORMATS):
            for mode, with_g in MODES:
                S = Sized.of(sizes, fmt, ao_format, aos, seed=300 + 10 * fmt, shift=k + mode)
                assert S.call(ao, mode, with_g) == 0, err(ao)
                S.check(mode, what=(fmt, mode))
                if mode != k % 3:
                    continue
                # one configuration per colour format: meao_composite_format per frame, on a reserved context resized to each frame's
                # size, leaves the same bytes on copies of the inputs
                R = Sized.of(sizes, fmt, ao_format, aos, seed=300 + 10 * fmt, shift=k + mode)
                for T in R.Ts:
                    ref.resize(T.w, T.h)
                    rc = ref._lib.meao_composite_format(ref._ctx, mode, T.ao_ptrs()[0], T.ao_pitch, T.color_ptrs()[0], fmt, T.color_pitch,
                                                        T.g_ptrs()[0] if mode == 1 else None, T.g_pitch, L.MEM_DEVICE, None)
                    assert rc == 0, err(ref)
                torch.cuda.synchronize()
                for f, (A, B) in enumerate(zip(S.Ts, R.Ts)):
                    assert torch.equal(A.color.dev, B.color.dev) and torch.equal(A.g.dev, B.g.dev), (fmt, mode, f)
    finally:
        ao.close()
        ref.close()


# ---- row and lane edges: the smallest shapes where the row form can go wrong

LONG_ROW = {CF.RGBA16F: (515, 3), CF.RGBA32F: (259, 3), CF.RGBA8: (1030, 3), CF.R11G11B10F: (1030, 3)}     # more than 256 lane-loads a row


@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_row_and_lane_edges(oracle, fmt, ao_format):
    rng = np.random.default_rng(11 + fmt)
    edges = [(1, 7), (7, 1), (2, 1), (64, 3), (65, 3), (66, 3), (67, 3), LONG_ROW[fmt]]
    ao = big_context(oracle, ao_format)
    try:
        for mode, with_g in MODES:
            for sizes in (edges, [(1, 1), CTX], [CTX, (1, 1)]):      # ... and a grid whose x is far beyond the small frame's rows
                aos = [random_ao(rng, w, h, ao_format) for w, h in sizes]
                S = Sized.of(sizes, fmt, ao_format, aos, seed=400 + mode, shift=mode)
                assert S.call(ao, mode, with_g) == 0, err(ao)
                S.check(mode, what=(fmt, mode, len(sizes)))
    finally:
        ao.close()


# ---- per-frame forms

@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_one_misaligned_frame_keeps_its_neighbours_form(oracle, fmt):
    """Frames 0, 1, 3 at vector-eligible origins and pitches, frame 2 one AO texel and 4 colour bytes (plus one texel) off with an
    odd stride in texels.  Which form a frame ran cannot be seen from here (the launcher chooses `vec` per frame); every frame must
    be exact and its guards intact."""
    sizes = [(255, 31), (400, 272), (67, 49), (96, 64)]
    rng = np.random.default_rng(5)
    ao = big_context(oracle)
    try:
        for mode, with_g in MODES:
            Ts = []
            for f, (w, h) in enumerate(sizes):
                a = random_ao(rng, w, h, L.AO_R8)
                if f != 2:
                    Ts.append(FormatTargets(w, h, fmt, L.AO_R8, "vector", [a], seed=500 + f))
                    continue
                odd = (w + 4) | 1
                g = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
                Ts.append(Targets(w, h, fmt, L.AO_R8, "odd", (((1, odd), (1, odd), (3, w + 5)), Y0, h + Y0 + 1, 4), [a],
                                  [random_color(rng, fmt, h, w)], [g]))
            S = Sized(Ts)
            assert S.call(ao, mode, with_g) == 0, err(ao)
            S.check(mode, what=(fmt, mode))
    finally:
        ao.close()


# ---- table bounds

@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_table_bounds_at_max_batch(ao_format):
    """n = max_batch = MEAO_MAX_BATCH with 64 different sizes: every entry of the table, every frame its own random AO and colours."""
    from miniengineao_amd import AmbientOcclusion
    n = L.MAX_BATCH
    sizes = [(8 + f, 5 + f % 7) for f in range(n)]
    rng = np.random.default_rng(3)
    aos = [random_ao(rng, w, h, ao_format) for w, h in sizes]
    ao = AmbientOcclusion(34, 18, max_batch=n, ao_format=ao_format)
    try:
        for fmt, mode in ((CF.RGBA16F, 0), (CF.RGBA8, 1), (CF.R11G11B10F, 0), (CF.RGBA32F, 2)):
            S = Sized.of(sizes, fmt, ao_format, aos, seed=600 + 100 * fmt)
            assert S.call(ao, mode) == 0, err(ao)
            S.check(mode, what=(fmt, mode))
        S = Sized.of(sizes, CF.RGBA8, ao_format, aos, seed=1000)
        assert S.call(ao, 0, n=n + 1) == L.ERR_INVALID_ARGUMENT
        assert "meao_composite_batch_extents" in err(ao) and "n must be" in err(ao), err(ao)
        S.check(0, frames=())
    finally:
        ao.close()


# ---- both rings

def test_both_rings_wrap_with_the_host_ahead():
    """20 calls on one stream with nothing waited for in between, alternating meao_composite_batch and meao_composite_batch_extents
    (n = 1..3, every call its own surfaces, formats and layouts cycling): each ring of 8 slots wraps with the host ahead.  A wrong
    entry stride or a slot refilled before its copy was consumed leaves wrong bytes in one particular call -- the one named."""
    from miniengineao_amd import AmbientOcclusion
    w, h, calls = 72, 40, 20
    rng = np.random.default_rng(8)
    ao = AmbientOcclusion(w, h, max_batch=3)
    try:
        work = []
        for k in range(calls):
            n, fmt = 1 + k % 3, ALL_FORMATS[k % 4]
            if k % 2 == 0:
                frames = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]
                work.append(FormatTargets(w, h, fmt, L.AO_R8, KINDS[k // 2 % 3], frames, seed=200 + k))
            else:
                sizes = [(w - 7 * f - k, h - 3 * f) for f in range(n)]
                work.append(Sized.of(sizes, fmt, L.AO_R8, [random_ao(rng, *s, L.AO_R8) for s in sizes], seed=200 + 10 * k, shift=k))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s = side.cuda_stream
        for k, T in enumerate(work):
            if k % 2 == 0:
                rc = ao._lib.meao_composite_batch(ao._ctx, 0, T.n, ptr_array(T.ao_ptrs()), T.ao_pitch, ptr_array(T.color_ptrs()), T.fmt,
                                                  T.color_pitch, None, 0, C.c_void_p(s))
            else:
                rc = T.call(ao, 0, stream=s)
            assert rc == 0, (k, err(ao))
        torch.cuda.synchronize()
        for k, T in enumerate(work):
            try:
                T.check(0)
            except AssertionError as e:
                raise AssertionError(f"call {k} of {calls} (n = {T.n}, slot {k // 2 % 8} of the {'sized' if k % 2 else 'uniform'} ring): {e}") from e
    finally:
        ao.close()


# ---- one launch

TRACE = r"""
import torch
from miniengineao_amd import AmbientOcclusion, _lib as L
sizes = [(33, 17), (97, 61), (400, 272), (66, 50), (67, 49)]
ao = AmbientOcclusion(400, 272, max_batch=8)
src = [torch.full((h, w), 128, dtype=torch.uint8, device="cuda") for w, h in sizes]
rgba8 = [torch.full((h, w, 4), 200, dtype=torch.uint8, device="cuda") for w, h in sizes]
depth = [torch.zeros((h, w), dtype=torch.float32, device="cuda") + 0.5 for w, h in sizes]
torch.cuda.synchronize()
ao.composite_tensors(src, rgba8, color_format=L.COLOR_RGBA8, batched=True)          # five frames of five sizes, one launch
torch.cuda.synchronize()
print("SIZED_DONE")
ao.execute_tensors(depth, color=rgba8, color_format=L.COLOR_RGBA8)                   # a shaded mixed call
torch.cuda.synchronize()
assert not ao.composite_pending
print("SHADED_DONE")
ao.close()
"""


def test_one_composite_launch_per_call(tmp_path):
    count = H.kernel_trace(tmp_path, TRACE)
    assert "SIZED_DONE" in count.stdout and "SHADED_DONE" in count.stdout
    comp = [i for i, k in enumerate(count.short) if k.startswith("composite_kernel")]
    assert len(comp) == 2 and count["render_with_composite_kernel"] == 0, count.short
    assert comp[0] == 0 and comp[1] == len(count.short) - 1, count.short        # the sized call; behind the last AO kernel of the shaded call
    assert len(count.short) >= 5 and any("_frames_kernel" in k for k in count.short[1:-1]), count.short       # ... which was a mixed call


# ---- meao_execute_batch_extents_shaded: AO = the oracle's at the frame's own size, colour = the model applied to that AO

class Shaded:
    """A MixedCall and colour targets for its frames: targets whose AO is the call's output surfaces."""

    def __init__(self, oracle, base, sizes, fmt, seed, per_frame=False, pitched=False, kinds=KINDS, call_seed=0):
        self.call = MixedCall(torch, oracle, base, sizes, per_frame=per_frame, pitched=pitched, seed=call_seed)
        self.fmt, self.n = fmt, len(sizes)
        self.Ts = [FormatTargets(w, h, fmt, base.ao_format, kinds[f % len(kinds)], [self.call.want(f)["result"]], seed=seed + f)
                   for f, (w, h) in enumerate(sizes)]

    def args(self, mode, with_g=True):
        c = self.call
        return dict(depth_ptrs=[d.ptr for d in c.depth], out_ptrs=[o.ptr for o in c.out], mode=mode,
                    color_ptrs=[T.color_ptrs()[0] for T in self.Ts],
                    gbuffer0_ptrs=[T.g_ptrs()[0] for T in self.Ts] if mode == 1 and with_g else None, params=c.params,
                    color_format=self.fmt, extents=c.extents, color_pitches=[T.color_pitch for T in self.Ts],
                    gbuffer0_pitches=[T.g_pitch for T in self.Ts])

    def run(self, ao, mode, **kw):
        ao.execute_shaded_device(**{**self.args(mode), **kw})

    def check(self, ao, mode, debug_buffers=False, what="", frames=None):
        self.call.check(ao, debug_buffers=False, what=what)
        if debug_buffers:                                   # frame 0, at its own size
            s0, want = self.call.settings[0], self.call.want(0)
            for i in H.valid_debug_ids(s0.num_levels, s0.hq_levels):
                got = ao.debug_buffer(i, frame=0)
                assert got.shape == want[H.NAMES[i]].shape, (what, H.NAMES[i], got.shape)
                assert H.nan_aware_equal(got, want[H.NAMES[i]])[0], (what, H.diff_report(H.NAMES[i], got, want[H.NAMES[i]]))
        for f, T in enumerate(self.Ts):
            try:
                T.check(mode, frames=(0,) if frames is None or f in frames else (), ao=T.ao.host)
            except AssertionError as e:
                raise AssertionError(f"{what} frame {f} ({T.w} x {T.h}, {T.kind}): {e}") from e

    def untouched(self):
        torch.cuda.synchronize()
        for f, o in enumerate(self.call.out):
            texels, intact = o.read()
            assert intact and np.all(texels.view(np.uint8) == M.SENTINEL), ("a refused call wrote AO", f)
        for T in self.Ts:
            T.check(0, frames=(), ao=T.ao.host)


@pytest.mark.parametrize("per_frame", [False, True])
def test_shaded_mixed_call(oracle, per_frame):
    base = base_settings(oracle)
    ao = context(base)
    try:
        for k, (fmt, (mode, _)) in enumerate(zip(ALL_FORMATS, MODES + MODES[:1])):
            S = Shaded(oracle, base, ORDER, fmt, seed=700 + 10 * k, per_frame=per_frame, pitched=bool(k % 2))
            S.run(ao, mode)
            assert not ao.composite_pending
            S.check(ao, mode, debug_buffers=(k == 0), what=(fmt, mode, per_frame))
    finally:
        ao.close()


@pytest.mark.parametrize("column", sorted(set(M.COLUMNS) - {"r8_rtz_exact"}) + ["exhaustive"])
def test_shaded_other_columns(oracle, column):
    kw = dict(sample_set=L.SAMPLES_EXHAUSTIVE) if column == "exhaustive" else M.COLUMNS[column]
    base = base_settings(oracle, **kw)
    ao = context(base)
    try:
        S = Shaded(oracle, base, [(33, 17), (200, 120), (97, 61)], CF.RGBA16F if "rtne" in column else CF.RGBA8, seed=800, per_frame=True)
        S.run(ao, 1)
        S.check(ao, 1, what=column)
    finally:
        ao.close()


# ---- state

def uniform_batch(oracle, base, n, seed):
    return MixedCall(torch, oracle, base, [CTX] * n, seed=seed)


def execute_uniform(ao, b):
    ao.execute_device([d.ptr for d in b.depth], [o.ptr for o in b.out])


def enqueue_waiting(ao, b, seed):
    """An RGBA16F composite of uniform batch b's AO, enqueued: -> (the colour tensors, their expected texels once it has run)."""
    before = [colour(*CTX, seed + f) for f in range(len(b.out))]
    col = [torch.from_numpy(c.view(np.int16).copy()).cuda() for c in before]
    ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [o.ptr for o in b.out], [c.data_ptr() for c in col])
    return col, before


def check_waiting(oracle, b, col, before, ran=True):
    torch.cuda.synchronize()
    for f in range(len(col)):
        want = before[f].copy()
        if ran:
            oracle.composite(np.ascontiguousarray(b.want(f)["result"]), want, L.COMPOSITE_MULTIPLY, L.AO_R8)
        assert np.array_equal(col[f].cpu().numpy().view(np.uint16), want), (f, ran)


def test_behind_an_announcement_and_with_a_ready_set(oracle):
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        nxt = uniform_batch(oracle, base, 2, seed=3)
        ao.prefetch_device([d.ptr for d in nxt.depth])
        S = Shaded(oracle, base, ORDER, CF.RGBA8, seed=900)
        S.run(ao, 0)
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, nxt)) == 0      # carried as a launch of its own, promoted, matched
        nxt.check(ao, debug_buffers=False, what="announced batch")
        S.check(ao, 0, what="carrying shaded call")
        # a ready set is consumed unmatched: the batch it was made for runs its own pass afterwards
        again = uniform_batch(oracle, base, 2, seed=4)
        ao.prefetch_device([d.ptr for d in again.depth])
        execute_uniform(ao, nxt)
        S2 = Shaded(oracle, base, ORDER, CF.R11G11B10F, seed=910)
        S2.run(ao, 0)
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, again)) > 0
        again.check(ao, debug_buffers=False, what="after the consumed set")
        S2.check(ao, 0, what="shaded call with a ready set")
    finally:
        ao.close()


def test_behind_a_waiting_enqueued_composite(oracle):
    base = base_settings(oracle)
    ao = context(base)
    try:
        b = uniform_batch(oracle, base, 2, seed=5)
        execute_uniform(ao, b)
        col, before = enqueue_waiting(ao, b, 70)
        assert pending(ao) == 2
        # the sized composite leaves it alone ...
        rng = np.random.default_rng(2)
        sizes = [(97, 61), (33, 17)]
        C1 = Sized.of(sizes, CF.RGBA32F, L.AO_R8, [random_ao(rng, w, h, L.AO_R8) for w, h in sizes], seed=920)
        assert C1.call(ao, 2) == 0, err(ao)
        assert pending(ao) == 2
        C1.check(2)
        check_waiting(oracle, b, col, before, ran=False)
        # ... the shaded mixed call runs it first
        S = Shaded(oracle, base, ORDER, CF.RGBA16F, seed=930)
        S.run(ao, 1)
        assert pending(ao) == 0
        S.check(ao, 1, what="shaded call behind a composite")
        check_waiting(oracle, b, col, before)
        # ... and after another sized composite a newly waiting batch is still carried by the next shared execute
        col, before = enqueue_waiting(ao, b, 75)
        C2 = Sized.of(sizes, CF.RGBA8, L.AO_R8, [random_ao(rng, w, h, L.AO_R8) for w, h in sizes], seed=940)
        assert C2.call(ao, 0) == 0 and pending(ao) == 2
        execute_uniform(ao, b)
        assert pending(ao) == 0
        C2.check(0)
        check_waiting(oracle, b, col, before)
    finally:
        ao.close()


def test_under_a_reservation_the_capacity_bounds_the_call(oracle):
    base = base_settings(oracle)
    ao = context(base)
    try:
        ao.reserve(*CTX)
        ao.resize(200, 120)
        S = Shaded(oracle, base, ORDER, CF.RGBA8, seed=950, per_frame=True)
        S.run(ao, 1)
        S.check(ao, 1, what="reserved")
        assert (ao.width, ao.height) == (200, 120) and ao.capacity == CTX
    finally:
        ao.close()


# ---- uniform collapse

def test_uniform_extents_are_the_uniform_calls(oracle):
    base = base_settings(oracle)
    ao = context(base)
    try:
        for fmt, kind in ((CF.RGBA16F, "packed"), (CF.RGBA8, "vector")):
            b = uniform_batch(oracle, base, 2, seed=5)
            aos = [b.want(f)["result"] for f in range(2)]
            # the composite: equal extents and shared strides against meao_composite_batch on copies
            A = FormatTargets(*CTX, fmt, L.AO_R8, kind, aos, seed=960)
            B = FormatTargets(*CTX, fmt, L.AO_R8, kind, aos, seed=960)
            ext = target_extents_array([(*CTX, A.ao_pitch, A.color_pitch, A.g_pitch)] * 2, 2)
            assert ao._lib.meao_composite_batch_extents(ao._ctx, 1, 2, ptr_array(A.ao_ptrs()), ptr_array(A.color_ptrs()), fmt,
                                                        ptr_array(A.g_ptrs()), ext, None) == 0, err(ao)
            assert ao._lib.meao_composite_batch(ao._ctx, 1, 2, ptr_array(B.ao_ptrs()), B.ao_pitch, ptr_array(B.color_ptrs()), fmt, B.color_pitch,
                                                ptr_array(B.g_ptrs()), B.g_pitch, None) == 0, err(ao)
            A.check(1)
            assert torch.equal(A.color.dev, B.color.dev) and torch.equal(A.g.dev, B.g.dev), fmt
            # the same sizes with two different colour strides: the sized launch, the same bytes
            S = Sized([FormatTargets(*CTX, fmt, L.AO_R8, k, [a], seed=970 + f) for f, (k, a) in enumerate(zip(("packed", "vector"), aos))])
            assert S.call(ao, 1) == 0, err(ao)
            S.check(1, what="two strides")
            # the shaded call: uniform extents against meao_execute_batch_shaded
            X, Y = (FormatTargets(*CTX, fmt, L.AO_R8, kind, aos, seed=980) for _ in range(2))
            out2 = [torch.zeros((CTX[1], CTX[0]), dtype=torch.uint8, device="cuda") for _ in range(2)]
            d = [s.ptr for s in b.depth]
            ao.execute_shaded_device(d, [o.ptr for o in b.out], 0, X.color_ptrs(), color_format=fmt, extents=[CTX] * 2,
                                     color_pitches=[X.color_pitch] * 2)
            ao.execute_shaded_device(d, [o.data_ptr() for o in out2], 0, Y.color_ptrs(), color_format=fmt, color_pitch=Y.color_pitch)
            b.check(ao, debug_buffers=False, what="uniform shaded")
            X.check(0, ao=X.ao.host)
            assert torch.equal(X.color.dev, Y.color.dev), fmt
            for f in range(2):
                assert np.array_equal(out2[f].cpu().numpy(), aos[f]), f
    finally:
        ao.close()


# ---- refusals: the documented status, the call, the frame and the argument named, nothing launched

def test_refusals(oracle):
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        b = uniform_batch(oracle, base, 2, seed=5)
        execute_uniform(ao, b)
        col, before = enqueue_waiting(ao, b, 80)
        ao.synchronize()
        S = Shaded(oracle, base, ORDER, CF.RGBA8, seed=990, kinds=("vector",))      # ORDER[1] = 400 x 272, ORDER[2] = 200 x 120
        good = S.args(0)
        INV, UNS = L.ERR_INVALID_ARGUMENT, L.ERR_UNSUPPORTED

        def with_pitch(f, pitch, key="color_pitches"):
            p = list(good[key])
            p[f] = pitch
            return {key: p}

        def with_extent(f, e):
            x = list(good["extents"])
            x[f] = e
            return dict(extents=x)

        def without(key, f):
            p = list(good[key])
            p[f] = None
            return {key: p}

        shaded_cases = [
            (INV, [r"extents\[2\]", "width/height"], with_extent(2, (401, 120, 0, 0))),            # beyond the capacity
            (INV, [r"extents\[0\]", "width/height"], with_extent(0, (0, 17, 0, 0))),
            (INV, [r"extents\[0\]", "width/height"], with_extent(0, (32769, 17, 0, 0))),
            (INV, [r"color_pitch\[2\]", "smaller than a row"], with_pitch(2, 160 * 4)),               # enough for frame 0's 33 texels
            (INV, [r"color_pitch\[3\]", "multiple of the element size"], with_pitch(3, good["color_pitches"][3] + 2)),
            (UNS, [r"color_pitch\[0\]", "2\\^24"], with_pitch(0, 4 << 24)),
            (UNS, [r"color_pitch\[1\]", "2\\^32 - 1"], with_pitch(1, 16_000_000)),                       # 271 rows x 16 MB
            (INV, ["gbuffer0_rgba8", "AMBIENT_ONLY"], dict(mode=1, gbuffer0_ptrs=None)),
            (INV, ["frame 1", "color", "null"], without("color_ptrs", 1)),
            (INV, ["color_format"], dict(color_format=7)),
            (INV, [r"extents\[3\]\.depth_pitch"], with_extent(3, (97, 61, 96 * 4, 0))),               # the execute half, under this name
            (INV, [r"params\[1\]"], dict(params=[None, dataclasses.replace(H.params_of(S.call.settings[1]), intensity=float("nan")), None, None])),
        ]
        for status, words, kw in shaded_cases:
            with pytest.raises(L.MeaoError) as e:
                ao.execute_shaded_device(**{**good, **kw})
            assert e.value.status == status, (kw, str(e.value))
            for word in ["meao_execute_batch_extents_shaded"] + words:
                assert re.search(word, str(e.value)), (word, str(e.value))

        # the composite alone: the same surfaces, the AO frames being the (untouched) outputs
        Z = Sized(S.Ts)
        aos = [o.ptr for o in S.call.out]
        ext = [(w, h, o.pitch_bytes, T.color_pitch, T.g_pitch) for (w, h), o, T in zip(ORDER, S.call.out, S.Ts)]

        def ext_with(f, **kw):
            x = list(ext)
            e = dict(zip(("w", "h", "ao", "color", "g"), x[f]))
            e.update(kw)
            x[f] = tuple(e.values())
            return dict(extents=x)

        colors = Z.color_ptrs()
        composite_cases = [
            (INV, [r"extents\[0\]", "width/height"], ext_with(0, w=0)),
            (INV, [r"extents\[0\]", "width/height"], ext_with(0, w=32769)),
            (INV, [r"extents\[2\]\.color_pitch", "smaller than a row"], ext_with(2, color=160 * 4)),
            (INV, [r"extents\[3\]\.color_pitch", "multiple of the element size"], ext_with(3, color=ext[3][3] + 2)),
            (INV, [r"extents\[3\]\.ao_pitch", "smaller than a row"], ext_with(3, ao=96)),
            (UNS, [r"extents\[0\]\.color_pitch", "2\\^24"], ext_with(0, color=4 << 24)),
            (UNS, [r"extents\[1\]\.color_pitch", "2\\^32 - 1"], ext_with(1, h=32768, color=262144)),     # arguments only: nothing is launched
            (UNS, [r"extents\[1\]\.color_pitch", "2\\^32 - 1", "packed"], ext_with(1, w=32768, h=32768, ao=0, color=0, g=0)),   # packed rows too
            (INV, ["gbuffer0_rgba8", "AMBIENT_ONLY"], dict(mode=1, with_g=False)),
            (INV, ["frame 1", "color", "null"], dict(colors=[colors[0], None] + colors[2:])),
            (INV, ["color_format"], dict(fmt=-1)),
            (INV, ["n must be"], dict(n=MAX_BATCH + 1)),
        ]
        for status, words, kw in composite_cases:
            kw = {**dict(mode=0, aos=aos, extents=ext), **kw}
            assert Z.call(ao, **kw) == status, (kw, err(ao))
            for word in ["meao_composite_batch_extents"] + words:
                assert re.search(word, err(ao)), (word, err(ao))

        # nothing ran: AO and colours as they were, the batch still waits and is carried by the next shared execute
        S.untouched()
        assert pending(ao) == 2
        check_waiting(oracle, b, col, before, ran=False)
        execute_uniform(ao, b)
        assert pending(ao) == 0
        check_waiting(oracle, b, col, before)
        # ... and the valid call still works
        ao.execute_shaded_device(**good)
        S.check(ao, 0, what="after the refusals")
    finally:
        ao.close()


# ---- the pool

@pytest.mark.parametrize("members", [2, 3])
def test_pool(oracle, members):
    from miniengineao_amd import AmbientOcclusionPool
    base = base_settings(oracle)
    sizes = [(33, 17), (400, 272), (97, 61), (97, 61), (129, 65)]      # five frames of four sizes; n no multiple of 2 or 3
    pool = AmbientOcclusionPool(*CTX, [0] * members, max_batch=MAX_BATCH, near_clip=base.near_clip, far_clip=base.far_clip,
                                projection00=base.proj00, reversed_z=base.reversed_z, pipelined=True)
    try:
        for per_frame, fmt, mode in ((False, CF.RGBA8, 1), (True, CF.RGBA16F, 0)):
            S = Shaded(oracle, base, sizes, fmt, seed=1100, per_frame=per_frame)
            pool.execute_shaded_device(**S.args(mode))
            assert not pool.composite_pending
            pool.synchronize()
            S.check(pool, mode, what=(members, per_frame))
        # an invalid frame 4 refuses the call before any member enqueues
        S = Shaded(oracle, base, sizes, CF.RGBA8, seed=1200)
        bad = S.args(0)
        bad["color_pitches"][4] = 128 * 4
        with pytest.raises(L.MeaoError, match=r"meao_pool_execute_batch_extents_shaded: member %d .*color_pitch\[%d\]" % (4 % members, 4 // members)) as e:
            pool.execute_shaded_device(**bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        pool.synchronize()
        S.untouched()
        # a member dealt nothing drops its announcement.  One frame is announced to every member, then a shaded call of one frame
        # passes the last member by.  Had it kept the announcement, call X below would carry it and leave a ready set keyed on its
        # frame, and call Y on the same pointers would find its downsample pass done.
        nxt = uniform_batch(oracle, base, members, seed=3)
        ptrs = ([d.ptr for d in nxt.depth], [o.ptr for o in nxt.out])
        pool.prefetch_device(ptrs[0])
        one = Shaded(oracle, base, [(97, 61)], CF.RGBA8, seed=1300)
        pool.execute_shaded_device(**one.args(0))
        pool.execute_device(*ptrs)                                     # X
        pool.synchronize()
        one.check(pool, 0, what="one frame")
        last = pool.member_context(members - 1)
        L.check(pool._lib.meao_set_profiling(last, 1))
        pool.execute_device(*ptrs)                                     # Y
        pool.synchronize()
        ms, cnt = (C.c_float * L.NUM_PASSES)(), C.c_int32()
        L.check(pool._lib.meao_get_pass_times(last, C.byref(ms), C.byref(cnt)))
        assert cnt.value == 1 and ms[H.PASS_DOWNSAMPLE] > 0, list(ms)
    finally:
        pool.close()


# ---- the tensor forms

def test_tensor_forms_on_lists_of_different_shapes(oracle):
    base = base_settings(oracle)
    ao = context(base)
    rng = np.random.default_rng(6)
    try:
        depth, color, color2, gbuf, raw_c, raw_g, wants = [], [], [], [], [], [], []
        for f, (w, h) in enumerate(ORDER):
            raw, _ = M.frame(oracle, w, h)
            s = M.frame_settings(base, w, h)
            wants.append(H.want_of(oracle, (w, h, M.F32, False, 0), raw, s, nthreads=8)["result"])
            rc, rg = rng.integers(0, 256, (h + 3, w + 6, 4), dtype=np.uint8), rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            raw_c.append(rc)
            raw_g.append(rg)
            if f % 2:                                                  # two crops of larger tensors
                surface = torch.full((h + 3, w + 5 + f), 0.25, dtype=torch.float32, device="cuda")
                surface[1:1 + h, 2:2 + w] = torch.from_numpy(raw).cuda()
                depth.append(surface[1:1 + h, 2:2 + w])
                color.append(torch.from_numpy(rc.copy()).cuda()[2:2 + h, 4:4 + w])
                color2.append(torch.from_numpy(rc.copy()).cuda()[2:2 + h, 4:4 + w])
            else:
                depth.append(torch.from_numpy(raw).cuda())
                color.append(torch.from_numpy(rc[2:2 + h, 4:4 + w].copy()).cuda())
                color2.append(torch.from_numpy(rc[2:2 + h, 4:4 + w].copy()).cuda())
            gbuf.append(torch.from_numpy(rg.copy()).cuda())
        outs = ao.execute_tensors(depth, color=color, gbuffer0=gbuf, mode=L.COMPOSITE_AMBIENT_ONLY, color_format=L.COLOR_RGBA8)
        ao.composite_tensors(outs, color2, color_format=L.COLOR_RGBA8, batched=True)
        torch.cuda.synchronize()
        for f, (w, h) in enumerate(ORDER):
            assert tuple(outs[f].shape) == (h, w) and np.array_equal(outs[f].cpu().numpy(), wants[f]), f
            view = raw_c[f][2:2 + h, 4:4 + w]
            want_c, want_g = CF.composite(wants[f], L.AO_R8, view, CF.RGBA8, 1, raw_g[f])
            assert np.array_equal(color[f].cpu().numpy(), want_c) and np.array_equal(gbuf[f].cpu().numpy(), want_g), f
            assert np.array_equal(color2[f].cpu().numpy(), CF.composite(wants[f], L.AO_R8, view, CF.RGBA8, 0)[0]), f
            if f % 2:                                                  # the bytes around a crop stay
                whole = color[f]._base.cpu().numpy() if color[f]._base is not None else None
                want = raw_c[f].copy()
                want[2:2 + h, 4:4 + w] = want_c
                assert whole is not None and np.array_equal(whole, want), f
        with pytest.raises(ValueError):
            ao.execute_tensors(depth, gbuffer0=gbuf)
    finally:
        ao.close()
