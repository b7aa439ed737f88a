"""The batch in one launch (meao_composite_batch) and shaded frames from the execute call (meao_execute_batch_shaded, the pool form,
execute_tensors(color=), composite_tensors(batched=True)) on the GPU.

Expected colours never come from the library: RGBA16F from the oracle (oracle.run + oracle.composite), the other formats from the
NumPy model tests/color_formats.py.  A second assertion in each case compares with the per-frame meao_composite_format on copies of
the same inputs.  Surfaces are the Targets of tests/test_composite_formats_gpu.py: viewports inside 0xA5-filled allocations, every
byte outside a viewport unchanged afterwards (layouts "packed", "vector", "oddbase" = origins one AO texel / 4 colour bytes off:
the per-texel form for the whole batch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from miniengineao_amd import _lib as L
from miniengineao_amd import synth
from miniengineao_amd.frame_params import FrameParams, params_array
from tests import color_formats as CF
from tests import helpers as H
from tests.composite_targets import FormatTargets as BatchTargets
from tests.helpers import encode_depth as encode
from tests.helpers import frame_settings, oracle_frame, ptr_array

pytestmark = pytest.mark.gpu

ALL_FORMATS = [CF.RGBA16F, CF.RGBA32F, CF.RGBA8, CF.R11G11B10F]
MODES = ((0, False), (1, True), (2, False))


def stream():
    return torch.cuda.current_stream().cuda_stream


def batch(ao, T, mode, with_g=True, n=None, stream_=None):
    n = T.n if n is None else n
    return ao._lib.meao_composite_batch(ao._ctx, mode, n, ptr_array(T.ao_ptrs()), T.ao_pitch, ptr_array(T.color_ptrs()), T.fmt, T.color_pitch,
                                        ptr_array(T.g_ptrs()) if mode == 1 and with_g else None, T.g_pitch,
                                        C.c_void_p(stream() if stream_ is None else stream_))


def per_frame(ao, T, mode, with_g=True):
    a, c, g = T.ao_ptrs(), T.color_ptrs(), T.g_ptrs()
    for f in range(T.n):
        rc = ao._lib.meao_composite_format(ao._ctx, mode, a[f], T.ao_pitch, c[f], T.fmt, T.color_pitch, g[f] if mode == 1 and with_g else None,
                                           T.g_pitch, L.MEM_DEVICE, C.c_void_p(stream()))
        assert rc == 0, ao._lib.meao_last_error(ao._ctx)


def err(ao):
    return ao._lib.meao_last_error(ao._ctx).decode()


def same_as_per_frame(ao, T, mode, with_g, seed):
    """The second assertion: the per-frame entry point on copies of the same inputs leaves the same bytes."""
    B = BatchTargets(T.w, T.h, T.fmt, T.ao_format, T.kind, T.want_ao, seed=seed)
    per_frame(ao, B, mode, with_g)
    torch.cuda.synchronize()
    assert torch.equal(T.color.dev, B.color.dev) and torch.equal(T.g.dev, B.g.dev), (T.kind, T.fmt, mode)


# ---- shapes x layouts x formats x modes x AO formats x n

@pytest.mark.parametrize("kind", ["packed", "vector", "oddbase"])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(66, 50), (67, 49)])          # odd pair count, a half pair, W mod 4 = 2 and 3
@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_shapes_and_layouts(oracle, ao_format, w, h, n, kind):
    frames = [oracle_frame(oracle, w, h, ao_format, 40 + f)[1] for f in range(n)]          # every frame its own AO and colours
    ao = H.component(H.settings(oracle, w, h, ao_format=ao_format), max_batch=5)
    try:
        for fmt in ALL_FORMATS:
            for mode, with_g in MODES:
                T = BatchTargets(w, h, fmt, ao_format, kind, frames, seed=23 + fmt)
                assert batch(ao, T, mode, with_g) == 0, err(ao)
                T.check(mode)
                same_as_per_frame(ao, T, mode, with_g, 23 + fmt)
    finally:
        ao.close()


@pytest.mark.parametrize("fmt", ALL_FORMATS)
def test_one_misaligned_frame_takes_the_whole_batch_to_the_scalar_form(oracle, fmt):
    """Frames 0, 1, 3 at vector-eligible origins, frame 2 one AO texel / 4 colour bytes off with the same pitches."""
    w, h = 67, 49
    frames = [oracle_frame(oracle, w, h, L.AO_R8, 40 + f)[1] for f in range(4)]
    ao = H.component(H.settings(oracle, w, h), max_batch=4)
    try:
        for mode in (0, 2):                                      # (the two layouts differ in their GBuffer0 pitch)
            A = BatchTargets(w, h, fmt, L.AO_R8, "vector", [frames[0], frames[1], frames[3]], seed=31)
            B = BatchTargets(w, h, fmt, L.AO_R8, "oddbase", [frames[2]], seed=32)
            assert (A.ao_pitch, A.color_pitch) == (B.ao_pitch, B.color_pitch)
            a, c = A.ao_ptrs(), A.color_ptrs()
            a.insert(2, B.ao_ptrs()[0])
            c.insert(2, B.color_ptrs()[0])
            rc = ao._lib.meao_composite_batch(ao._ctx, mode, 4, ptr_array(a), A.ao_pitch, ptr_array(c), fmt, A.color_pitch, None, 0,
                                              C.c_void_p(stream()))
            assert rc == 0, err(ao)
            A.check(mode)
            B.check(mode)
    finally:
        ao.close()


@pytest.mark.parametrize("ao_format", [L.AO_R8, L.AO_F16])
def test_table_bounds_at_max_batch(ao_format):
    """n = max_batch = MEAO_MAX_BATCH: every entry of the table, every frame its own random AO and colours."""
    from miniengineao_amd import AmbientOcclusion
    n, w, h = L.MAX_BATCH, 34, 18
    rng = np.random.default_rng(3)
    if ao_format == L.AO_R8:
        frames = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]
    else:
        frames = [rng.random((h, w)).astype(np.float16).view(np.uint16) for _ in range(n)]
    ao = AmbientOcclusion(w, h, max_batch=n, ao_format=ao_format)
    try:
        for fmt, mode, kind in ((CF.RGBA16F, 0, "packed"), (CF.RGBA8, 1, "vector"), (CF.R11G11B10F, 0, "oddbase"), (CF.RGBA32F, 2, "vector")):
            T = BatchTargets(w, h, fmt, ao_format, kind, frames, seed=50 + fmt)
            assert batch(ao, T, mode) == 0, err(ao)
            T.check(mode)
            same_as_per_frame(ao, T, mode, True, 50 + fmt)
        T = BatchTargets(w, h, CF.RGBA8, ao_format, "packed", frames, seed=60)
        assert ao._lib.meao_composite_batch(ao._ctx, 0, n + 1, ptr_array(T.ao_ptrs() + [0]), 0, ptr_array(T.color_ptrs() + [0]), T.fmt, 0, None,
                                            0, None) == L.ERR_INVALID_ARGUMENT
        T.check(0, frames=())
    finally:
        ao.close()


def test_ring_of_composite_tables_wraps_with_the_host_ahead():
    """20 meao_composite_batch calls on one stream with nothing waited for in between: the ring of 8 table slots wraps twice with
    the host running ahead.  Every call has its own AO and colours (n = 1..3 of max_batch 3, formats and layouts cycling; 72 x 40:
    pitched rows that do not fill a workgroup's row of lanes), so a launch that read another call's table entries, or a slot
    refilled before its copy was consumed, leaves wrong bytes in one particular call -- the one the failure names."""
    from miniengineao_amd import AmbientOcclusion
    w, h, calls = 72, 40, 20
    rng = np.random.default_rng(8)
    ao = AmbientOcclusion(w, h, max_batch=3)
    try:
        Ts = []
        for k in range(calls):
            frames = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(1 + k % 3)]
            Ts.append(BatchTargets(w, h, ALL_FORMATS[k % 4], L.AO_R8, ("packed", "vector", "oddbase")[k // 3 % 3], frames, seed=200 + k))
        torch.cuda.synchronize()
        s = stream()
        for k, T in enumerate(Ts):
            assert batch(ao, T, 0, stream_=s) == 0, (k, err(ao))
        torch.cuda.synchronize()
        for k, T in enumerate(Ts):
            try:
                T.check(0)
            except AssertionError as e:
                raise AssertionError(f"call {k} of {calls} (n = {T.n}, table slot {k % 8}): {e}") from e
    finally:
        ao.close()


# ---- launch counts

TRACE = r"""
import ctypes as C, torch
from miniengineao_amd import AmbientOcclusion, _lib as L
from miniengineao_amd.frame_params import FrameParams
w, h = 640, 360
ao = AmbientOcclusion(w, h, max_batch=5)
depth = torch.zeros((5, h, w), dtype=torch.float32, device="cuda") + 0.5
out = torch.zeros((5, h, w), dtype=torch.uint8, device="cuda")
src = torch.full((5, h, w), 128, dtype=torch.uint8, device="cuda")
packed = torch.zeros((5, h, w), dtype=torch.int32, device="cuda")
rgba8 = torch.full((3, h, w, 4), 200, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
s = torch.cuda.current_stream().cuda_stream
ao.composite_tensors(src, packed, color_format=L.COLOR_R11G11B10F, batched=True)            # five frames, one launch
torch.cuda.synchronize()
print("BATCH_DONE")
fps = [FrameParams(intensity=1.0 + 0.5 * f) for f in range(3)]
ao.execute_tensors(depth[:3], out=out[:3], params=fps, color=rgba8, color_format=L.COLOR_RGBA8)
torch.cuda.synchronize()
assert not ao.composite_pending
print("SHADED_DONE")
ao.execute_tensors(depth[:3], out=out[:3], params=fps)
ao.composite_tensors(out[:3], rgba8, enqueue=True, color_format=L.COLOR_RGBA8)               # the old way: still one launch per frame
ao.execute_tensors(depth[:3], out=out[:3], params=fps)
torch.cuda.synchronize()
assert not ao.composite_pending
ao.close()
"""

PLAIN = r"""
import torch
from miniengineao_amd import AmbientOcclusion
from miniengineao_amd.frame_params import FrameParams
w, h = 640, 360
ao = AmbientOcclusion(w, h, max_batch=5)
depth = torch.zeros((3, h, w), dtype=torch.float32, device="cuda") + 0.5
out = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
ao.execute_tensors(depth, out=out, params=[FrameParams(intensity=1.0 + 0.5 * f) for f in range(3)])
torch.cuda.synchronize()
ao.close()
"""


def test_launch_counts(tmp_path):
    count = H.kernel_trace(tmp_path, TRACE)
    (tmp_path / "plain").mkdir()
    plain = H.kernel_trace(tmp_path / "plain", PLAIN)
    assert "BATCH_DONE" in count.stdout and "SHADED_DONE" in count.stdout
    assert count["render_with_composite_kernel"] == 0, count
    comp = [i for i, k in enumerate(count.short) if k.startswith("composite_kernel")]
    # one for the five R11G11B10F frames, one for the shaded call, three for the enqueued RGBA8 batch that the last execute runs first
    assert len(comp) == 1 + 1 + 3, count.short
    assert comp[0] == 0, count.short
    # the shaded call: the AO kernels of meao_execute_batch_params, then exactly one composite_kernel behind the last of them
    execute = plain.short
    assert len(execute) >= 3 and not any(k.startswith("composite_kernel") for k in execute), execute
    assert count.short[1:1 + len(execute)] == execute, (count.short, execute)
    assert comp[1] == 1 + len(execute), count.short
    rest = count.short[comp[1] + 1:]
    assert rest == execute + ["composite_kernel<0>"] * 3 + execute, rest


# ---- meao_execute_batch_shaded: AO = the oracle's, colour = the model applied to that AO

WS, HS = 96, 64


def own_params(n):
    return [FrameParams(intensity=1.0 + 0.5 * f, thicknessModifier=1.0 + f, blurTolerance=-4.6 + 0.5 * f) for f in range(n)]


class Scene:
    """n depth frames (in a 0xA5 / NaN-free padded surface when pitched), their oracle AO under per-frame settings, device buffers."""

    def __init__(self, oracle, base, n, params=None, depth_fmt=L.DEPTH_F32, pitched=False, seed=70, depths=None):
        self.n, self.pitched = n, pitched
        self.sets = [base if params is None else frame_settings(base, params[f]) for f in range(n)]
        self.depth = [encode(synth.make("S2", WS, HS, seed=seed + f), depth_fmt) for f in range(n)] if depths is None else depths
        self.want = [oracle.run(self.depth[f], self.sets[f], result_only=True)["result"] for f in range(n)]
        self.dp, self.op = (WS + 8, WS + 12) if pitched else (WS, WS)          # texels; both multiples of 4
        self.x0, self.y0, rows = (4, 1, HS + 2) if pitched else (0, 0, HS)     # where the frame sits in its surface
        dt = self.depth[0].dtype
        host = np.zeros((n, rows, self.dp), dt)
        host[:, self.y0:self.y0 + HS, self.x0:self.x0 + WS] = np.stack(self.depth)
        tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint16): torch.int16}[np.dtype(dt)]
        self.d = torch.from_numpy(host.view(np.int16) if tdt == torch.int16 else host).cuda()
        self.elem = host.itemsize
        self.out = torch.full((n, rows, self.op), 0xA5, dtype=torch.uint8, device="cuda")

    def depth_ptrs(self):
        return [self.d[f].data_ptr() + (self.y0 * self.dp + self.x0) * self.elem for f in range(self.n)]

    def out_ptrs(self):
        return [self.out[f].data_ptr() + self.y0 * self.op + self.x0 for f in range(self.n)]

    depth_pitch = property(lambda self: self.dp * self.elem if self.pitched else 0)
    out_pitch = property(lambda self: self.op if self.pitched else 0)

    def targets(self, fmt, kind, seed):
        """Colour targets whose AO pointers are this scene's outputs (the Targets' own AO surface stays an unused input; the AO
        pitch of a call is the scene's, whatever the layout of the colour)."""
        T = BatchTargets(WS, HS, fmt, L.AO_R8, kind, self.want, seed=seed)
        T.ao_ptrs = lambda base=None: self.out_ptrs()
        return T

    def shaded(self, ao, T, mode, params=None, n=None):
        n = self.n if n is None else n
        prm = None if params is None else params_array(params, n, ao._prm)
        ao._sync_params()
        return ao._lib.meao_execute_batch_shaded(ao._ctx, n, ptr_array(self.depth_ptrs()[:n]), self.depth_pitch, ptr_array(self.out_ptrs()[:n]),
                                                 self.out_pitch, prm, mode, ptr_array(T.color_ptrs()[:n]), T.fmt, T.color_pitch,
                                                 ptr_array(T.g_ptrs()[:n]) if mode == 1 else None, T.g_pitch, C.c_void_p(stream()))

    def check_ao(self, untouched=False):
        torch.cuda.synchronize()
        got = self.out.cpu().numpy()
        view = got[:, self.y0:self.y0 + HS, self.x0:self.x0 + WS]
        pad = np.ones(got.shape, bool)
        pad[:, self.y0:self.y0 + HS, self.x0:self.x0 + WS] = False
        assert (got[pad] == 0xA5).all(), "AO bytes outside the viewport changed"
        if untouched:
            assert (view == 0xA5).all(), "a refused call wrote AO"
            return
        for f in range(self.n):
            assert np.array_equal(view[f], self.want[f]), (f, H.diff_report("result", view[f], self.want[f]))


@pytest.mark.parametrize("case", ["shared", "per_frame", "unorm16", "pitched", "exhaustive"])
def test_execute_batch_shaded(oracle, case):
    n = 3
    fmt_d = L.DEPTH_UNORM16 if case == "unorm16" else L.DEPTH_F32
    kw = dict(depth_format=fmt_d)
    if case == "exhaustive":
        kw["sample_set"] = L.SAMPLES_EXHAUSTIVE
    base = H.settings(oracle, WS, HS, **kw)
    params = own_params(n) if case in ("per_frame", "pitched") else None
    S = Scene(oracle, base, n, params, fmt_d, pitched=case == "pitched")
    ao = H.component(base, max_batch=n, depth_format=fmt_d)
    try:
        for k, (fmt, mode, kind) in enumerate(((CF.RGBA16F, 0, "packed"), (CF.RGBA8, 1, "vector"), (CF.R11G11B10F, 0, "oddbase"),
                                               (CF.RGBA32F, 2, "vector"))):
            T = S.targets(fmt, kind, 80 + k)
            S.out.fill_(0xA5)
            assert S.shaded(ao, T, mode, params) == 0, err(ao)
            assert not ao.composite_pending
            S.check_ao()
            T.check(mode, ao=T.ao.host)
    finally:
        ao.close()


def test_execute_batch_shaded_with_an_announcement(oracle):
    """Three pipelined shaded steps: step k announces step k + 1, so step 1 consumes what step 0 carried and carries step 2's pass
    with the batched composite behind its last kernel; step 2, the one profiled, still finds its downsample done (no DOWNSAMPLE slot)."""
    n = 2
    base = H.settings(oracle, WS, HS)
    ao = H.component(base, max_batch=n, pipelined=True)
    try:
        steps = [Scene(oracle, base, n, seed=90 + 10 * k) for k in range(3)]
        Ts = [steps[k].targets(CF.RGBA8, "packed", 95 + k) for k in range(3)]
        torch.cuda.synchronize()
        for k in range(3):
            if k == 2:
                ao.set_profiling(True)
            if k + 1 < 3:
                ao.prefetch_device(steps[k + 1].depth_ptrs())
            assert steps[k].shaded(ao, Ts[k], 0) == 0, err(ao)
        ms, samples = ao.pass_times_ms()
        assert samples == 1 and ms[0] == 0 and ms[1] > 0, ms   # PASS_DOWNSAMPLE did not run in step 2: step 1 had carried it
        for k in range(3):
            steps[k].check_ao()
            Ts[k].check(0, ao=Ts[k].ao.host)
    finally:
        ao.close()


def test_execute_batch_shaded_sees_the_redone_lanes(oracle):
    """A NaN and a negative raw depth on odd texels: the full-resolution pass rewrites those lanes' AO after its vector store, and
    the composite behind it must read the final codes."""
    base = H.settings(oracle, WS, HS)
    d = synth.make("S2", WS, HS, seed=77).copy()
    d[21, 33], d[40, 57] = np.nan, -0.25
    S = Scene(oracle, base, 1, depths=[d])
    ao = H.component(base, max_batch=1)
    try:
        for k, fmt in enumerate((CF.RGBA16F, CF.RGBA8)):
            T = S.targets(fmt, "packed", 85 + k)
            S.out.fill_(0xA5)
            assert S.shaded(ao, T, 2) == 0, err(ao)           # DEBUG: the colour IS the AO
            S.check_ao()
            T.check(2, ao=T.ao.host)
    finally:
        ao.close()


# ---- state: a waiting batch

def test_a_waiting_batch_is_left_alone_then_carried(oracle):
    n = 3
    base = H.settings(oracle, WS, HS)
    S = Scene(oracle, base, n)
    ao = H.component(base, max_batch=n)
    try:
        ao.execute_device(S.depth_ptrs(), S.out_ptrs(), stream())
        W = S.targets(CF.RGBA16F, "packed", 101)                # waits for a render kernel
        assert ao._lib.meao_composite_enqueue_format(ao._ctx, 0, n, ptr_array(W.ao_ptrs()), 0, ptr_array(W.color_ptrs()), W.fmt, 0, None, 0) == 0
        pending = C.c_int32(0)
        assert ao._lib.meao_composite_pending(ao._ctx, C.byref(pending)) == 0 and pending.value == n
        other = S.targets(CF.R11G11B10F, "packed", 102)
        assert batch(ao, other, 0) == 0, err(ao)
        assert ao._lib.meao_composite_pending(ao._ctx, C.byref(pending)) == 0 and pending.value == n
        other.check(0, ao=other.ao.host)
        W.check(0, frames=(), ao=W.ao.host)                     # still waiting, untouched
        mine = S.targets(CF.RGBA8, "packed", 103)
        assert S.shaded(ao, mine, 0) == 0, err(ao)              # carries W as a plain execute would, and shades its own frames
        assert ao._lib.meao_composite_pending(ao._ctx, C.byref(pending)) == 0 and pending.value == 0
        S.check_ao()
        W.check(0, ao=W.ao.host)
        mine.check(0, ao=mine.ao.host)
    finally:
        ao.close()


# ---- refusals: the documented status, nothing launched, everything as it was

def test_refusals(oracle):
    n = 3
    base = H.settings(oracle, WS, HS)
    S = Scene(oracle, base, n, pitched=True)
    ao = H.component(base, max_batch=n, pipelined=True)
    try:
        ao.execute_device(S.depth_ptrs(), S.out_ptrs(), stream(), depth_pitch=S.depth_pitch, out_pitch=S.out_pitch)
        W = S.targets(CF.RGBA16F, "vector", 111)
        assert ao._lib.meao_composite_enqueue_format(ao._ctx, 0, n, ptr_array(W.ao_ptrs()), S.out_pitch, ptr_array(W.color_ptrs()), W.fmt,
                                                     W.color_pitch, None, 0) == 0
        torch.cuda.synchronize()
        S.out.fill_(0xA5)
        ao.prefetch_device(S.depth_ptrs(), depth_pitch=S.depth_pitch)
        T = S.targets(CF.RGBA8, "vector", 112)
        good = own_params(n)
        bad = params_array(good, n, ao._prm)
        bad[2].near_clip = float("nan")
        d, o, c, g = S.depth_ptrs(), S.out_ptrs(), T.color_ptrs(), T.g_ptrs()
        c_null = list(c)
        c_null[1] = None
        lib, ctx, s = ao._lib, ao._ctx, C.c_void_p(stream())

        def shaded(n_=n, mode=0, fmt=T.fmt, cp=T.color_pitch, colors=c, gb=None, prm=None):
            k = max(n_, n)
            pad = lambda p: ptr_array(list(p) + [p[0]] * (k - len(p)))
            return lib.meao_execute_batch_shaded(ctx, n_, pad(d), S.depth_pitch, pad(o), S.out_pitch, prm, mode, pad(colors), fmt, cp, gb,
                                                 T.g_pitch, s)

        def batched(n_=n, mode=0, fmt=T.fmt, cp=T.color_pitch, colors=c, gb=None):
            k = max(n_, n)
            pad = lambda p: ptr_array(list(p) + [p[0]] * (k - len(p)))
            return lib.meao_composite_batch(ctx, mode, n_, pad(W.ao_ptrs()), S.out_pitch, pad(colors), fmt, cp, gb, T.g_pitch, s)

        cases = [("n must be", dict(n_=0)), ("n must be", dict(n_=n + 1)), ("mode", dict(mode=-1)), ("mode", dict(mode=4)), ("color_format", dict(fmt=-1)),
                 ("color_format", dict(fmt=4)), ("GBuffer0", dict(mode=1)), ("color_pitch", dict(cp=WS * 4 - 4)),
                 ("color_pitch", dict(cp=T.color_pitch + 2)), ("null", dict(colors=c_null))]
        for call, name in ((shaded, "meao_execute_batch_shaded"), (batched, "meao_composite_batch")):
            for word, kw in cases:
                assert call(**kw) == L.ERR_INVALID_ARGUMENT, (name, kw)
                assert name in err(ao) and word in err(ao), (name, kw, err(ao))
        assert shaded(prm=bad) == L.ERR_INVALID_ARGUMENT
        assert "meao_execute_batch_shaded" in err(ao) and "params[2]" in err(ao), err(ao)
        # nothing ran: AO and colours as they were, the batch still waits
        S.check_ao(untouched=True)
        T.check(0, frames=(), ao=T.ao.host)
        W.check(0, frames=(), ao=W.ao.host)
        pending = C.c_int32(0)
        assert lib.meao_composite_pending(ctx, C.byref(pending)) == 0 and pending.value == n
        # ... and the announcement is still there: the next call runs the waiting batch and carries the announced frames' downsample
        # pass, so that the call after it finds the pass done
        assert shaded(prm=params_array(good, n, ao._prm)) == 0, err(ao)
        assert lib.meao_composite_pending(ctx, C.byref(pending)) == 0 and pending.value == 0
        ao.set_profiling(True)
        assert shaded(prm=params_array(good, n, ao._prm)) == 0, err(ao)
        ms, samples = ao.pass_times_ms()
        assert samples == 1 and ms[0] == 0, ms                 # PASS_DOWNSAMPLE: the announcement made before the refusals was honoured
    finally:
        ao.close()


# ---- pool

POOL_TRACE = r"""
import numpy as np, torch
from miniengineao_amd import AmbientOcclusionPool, _lib as L
w, h, n = 96, 64, 5
pool = AmbientOcclusionPool(w, h, [0, 0], max_batch=3)
depth = torch.zeros((n, h, w), dtype=torch.float32, device="cuda") + 0.5
out = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
color = torch.full((n, h, w, 4), 200, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
pool.execute_shaded_device([depth[f].data_ptr() for f in range(n)], [out[f].data_ptr() for f in range(n)], L.COMPOSITE_MULTIPLY,
                           [color[f].data_ptr() for f in range(n)], color_format=L.COLOR_RGBA8)
pool.synchronize()
pool.close()
"""


def test_pool_of_two_members(oracle, tmp_path):
    from miniengineao_amd import AmbientOcclusionPool
    n = 5
    base = H.settings(oracle, WS, HS)
    S = Scene(oracle, base, n)
    T = S.targets(CF.RGBA8, "packed", 121)
    pool = AmbientOcclusionPool(WS, HS, [0, 0], max_batch=3, near_clip=base.near_clip, far_clip=base.far_clip, projection00=base.proj00,
                                reversed_z=base.reversed_z)
    try:
        torch.cuda.synchronize()
        pool.execute_shaded_device(S.depth_ptrs(), S.out_ptrs(), 1, T.color_ptrs(), T.g_ptrs(), color_format=T.fmt)
        assert not pool.composite_pending
        pool.synchronize()
        S.check_ao()
        T.check(1, ao=T.ao.host)
        with pytest.raises(L.MeaoError, match="meao_pool_execute_batch_shaded"):
            pool.execute_shaded_device(S.depth_ptrs(), S.out_ptrs(), 1, T.color_ptrs(), None, color_format=T.fmt)
    finally:
        pool.close()
    count = H.kernel_trace(tmp_path, POOL_TRACE)
    assert count["composite_kernel"] == 2, count.short          # one batched launch per member (3 + 2 frames)


# ---- the tensor forms on crops

def test_tensor_forms_on_crops(oracle):
    n = 3
    base = H.settings(oracle, WS, HS)
    S = Scene(oracle, base, n)
    ao = H.component(base, max_batch=n)
    rng = np.random.default_rng(5)
    try:
        depth = torch.from_numpy(np.stack(S.depth)).cuda()
        ao_big = torch.full((n, HS + 5, WS + 12), 0xA5, dtype=torch.uint8, device="cuda")
        crop = ao_big[:, 3:3 + HS, 4:4 + WS]
        raw = rng.integers(0, 256, (n, HS + 4, WS + 8, 4), dtype=np.uint8)
        big = torch.from_numpy(raw.copy()).cuda()
        got_ao = ao.execute_tensors(depth, out=crop, color=big[:, 1:1 + HS, 4:4 + WS], color_format=L.COLOR_RGBA8)
        assert got_ao is crop
        big2 = torch.from_numpy(raw.copy()).cuda()
        ao.composite_tensors(crop, big2[:, 1:1 + HS, 4:4 + WS], color_format=L.COLOR_RGBA8, batched=True)
        torch.cuda.synchronize()
        want = raw.copy()
        for f in range(n):
            assert np.array_equal(crop[f].cpu().numpy(), S.want[f])
            want[f, 1:1 + HS, 4:4 + WS] = CF.composite(S.want[f], L.AO_R8, raw[f, 1:1 + HS, 4:4 + WS], CF.RGBA8, 0)[0]
        assert np.array_equal(big.cpu().numpy(), want) and np.array_equal(big2.cpu().numpy(), want)
        with pytest.raises(ValueError):
            ao.composite_tensors(crop, big2[:, 1:1 + HS, 4:4 + WS], color_format=L.COLOR_RGBA8, batched=True, enqueue=True)
    finally:
        ao.close()
