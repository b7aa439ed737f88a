"""AO parameters at the edges of the exact-division range and far outside the inspector ranges, on the GPU.

Under RTZ storage a context divides with the exact v_rcp_f32 sequences (DIV = 0) only while the upsample constants lie in the
range those were verified for (meao_api.cpp exact_rcp_div_applicable); any other finite value -- all of them valid inputs --
runs the IEEE-division bodies (DIV = 1), with a clamped, finite sky.  Each frame must equal the CPU oracle under its own
parameters in every buffer (NaN-aware), on both sides of each edge, far outside, in per-frame calls that mix the two, and
across the prefetch reuse key that depends on the column (ready_exact)."""
import os

import numpy as np
import pytest

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests import kernel_inventory as K
from tests.helpers import PASS_DOWNSAMPLE, flat_sky_frame, frame_settings, hostile_level_texels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HT = 516, 260
COLUMNS = {"r8_rtz": dict(), "r8_rtne": dict(f16_rounding=L.F16_RTNE), "f16_rtz": dict(ao_format=L.AO_F16),
           "f16_rtne": dict(ao_format=L.AO_F16, f16_rounding=L.F16_RTNE)}


def hostile_fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_s2h_516x260_hostile_r8.npz"))["depth"]


def check_frames(oracle, ao, depths, sets, ids=True):
    """Frame f of the last call against the oracle under sets[f]: the result and, with ids, every valid debug buffer."""
    for f, (d, s) in enumerate(zip(depths, sets)):
        want = oracle.run(d, s, nthreads=8)
        for i in H.valid_debug_ids(s.num_levels, s.hq_levels) if ids else [17]:
            got = ao.debug_buffer(i, frame=f)
            ok, _ = H.nan_aware_equal(got, want[H.NAMES[i]])
            assert ok, (f, i, H.diff_report(H.NAMES[i], got, want[H.NAMES[i]]))


# ---- both sides of each edge of the exact range; the child checks parity, the trace which column ran

EDGE_CHILD = r"""
import sys
import numpy as np
from oracle import oracle as O
from miniengineao_amd import _lib as L
from miniengineao_amd import synth
from tests import helpers as H
from tests.helpers import flat_sky_frame
from tests.test_param_domain_gpu import W, HT          # the child's own parent module, for these two constants alone

side = sys.argv[1]
lib = L.load()
O.build()
depths = [synth.make("S2", W, HT, seed=21), flat_sky_frame(W, HT, 22)]
for name, (field, inside, outside) in sorted(H.exact_range_edges(lib).items()):
    value = inside if side == "inside" else outside
    for ao_format in (L.AO_R8, L.AO_F16):
        s = H.settings(O, W, HT, ao_format=ao_format, **{field: value})
        ao = H.component(s, max_batch=2)
        try:
            ao.render_batch(depths)
            for f, d in enumerate(depths):
                want = O.run(d, s, nthreads=8)
                for i in H.valid_debug_ids(4):
                    got = ao.debug_buffer(i, frame=f)
                    if not H.nan_aware_equal(got, want[H.NAMES[i]])[0]:
                        sys.exit("%s %s=%r ao_format %d frame %d: %s" % (name, field, value, ao_format, f,
                                                                        H.diff_report(H.NAMES[i], got, want[H.NAMES[i]])))
        finally:
            ao.close()
print("edges ok", side)
"""


@pytest.mark.parametrize("side,div", [("inside", "0"), ("outside", "1")])
def test_exact_range_edges_every_buffer(tmp_path, side, div):
    k = H.kernel_trace(tmp_path, EDGE_CHILD, [side])
    cols = {K.column_of(n) for n in k.short} - {None}
    assert cols, k.short[:20]
    assert {c[2] if c[0] != "ds" else c[1] for c in cols} == {div}, (side, sorted(cols))
    assert {c for c in cols if c[0] != "ds"} == {("0", "false", div), ("1", "false", div)}, sorted(cols)


# ---- far outside the inspector ranges: overflow, underflow, zero, negative

@pytest.mark.parametrize("field,value", [(f, v) for f, vs in H.FAR_OUTSIDE.items() for v in vs])
def test_far_outside_every_column_every_buffer(oracle, field, value):
    depths = [synth.make("S2", W, HT, seed=31), flat_sky_frame(W, HT, 32), hostile_fixture()]
    for name, cfg in COLUMNS.items():
        s = H.settings(oracle, W, HT, **cfg, **{field: value})
        ao = H.component(s, max_batch=len(depths))
        try:
            ao.render_batch(depths)
            check_frames(oracle, ao, depths, [s] * len(depths))
        finally:
            ao.close()


# ---- per-frame calls mixing frames inside and outside the range: the whole call runs the IEEE bodies

MIXED_CHILD = r"""
import dataclasses
import sys
import numpy as np
import torch
from oracle import oracle as O
from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests.linear_depth import linearize, to_linear

O.build()
CAM = synth.Camera(near=0.1, far=128.0, reversed_z=True)
w, h = 384, 256
params = [FrameParams(intensity=1.5), FrameParams(upsampleTolerance=-14.0, thicknessModifier=3.0),
          FrameParams(noiseFilterTolerance=9.5), FrameParams(upsampleTolerance=-2.0, blurTolerance=-2.0)]
base = H.settings(O, w, h, cam=CAM)
sets = [dataclasses.replace(base, intensity=1.5), dataclasses.replace(base, upsample_tolerance=-14.0, thickness_modifier=3.0),
        dataclasses.replace(base, noise_filter_tolerance=9.5), dataclasses.replace(base, upsample_tolerance=-2.0, blur_tolerance=-2.0)]
raws = [synth.occluder_field(w, h, seed=40 + f, cam=CAM) for f in range(4)]
dev = torch.device("cuda", 0)


def check(ao, got, depths, what):
    for f, d in enumerate(depths):
        want = O.run(d, dataclasses.replace(sets[f], ao_format=ao.ao_format), nthreads=8)
        ok, _ = H.nan_aware_equal(got[f], want["result"])
        if not ok:
            sys.exit("%s frame %d: %s" % (what, f, H.diff_report("result", got[f], want["result"])))
        for i in H.valid_debug_ids(4) if f < 2 else []:
            g = ao.debug_buffer(i, frame=f)
            if not H.nan_aware_equal(g, want[H.NAMES[i]])[0]:
                sys.exit("%s frame %d: %s" % (what, f, H.diff_report(H.NAMES[i], g, want[H.NAMES[i]])))


for ao_format in (L.AO_R8, L.AO_F16):
    s = dataclasses.replace(base, ao_format=ao_format)
    ao = H.component(s, max_batch=4)                      # packed frames: the per-frame forms of the shared kernels
    check(ao, ao.render_batch(raws, params=params), raws, "per-frame")
    ao.close()
    ao = H.component(s, max_batch=4)                      # pitched surfaces
    dt = torch.uint8 if ao_format == L.AO_R8 else torch.float16
    surf = torch.full((4, h + 2, w + 8), float("nan"), dtype=torch.float32, device=dev)
    out = torch.zeros((4, h + 2, w + 8), dtype=dt, device=dev)
    for f in range(4):
        surf[f, 1:1 + h, 4:4 + w] = torch.from_numpy(raws[f]).to(dev)
    ao.execute_tensors(surf[:, 1:1 + h, 4:4 + w], out[:, 1:1 + h, 4:4 + w], params=params)
    torch.cuda.synchronize()
    o = out[:, 1:1 + h, 4:4 + w].cpu().numpy()
    check(ao, [o[f].view(np.uint8 if ao_format == L.AO_R8 else np.uint16) for f in range(4)], raws, "pitched")
    ao.close()
    lin_c = linearize()               # linear view-space depth
    pairs = [to_linear(lin_c, r, CAM) for r in raws]
    ao = H.component(s, max_batch=4, depth_format=L.DEPTH_LINEAR_F32)
    check(ao, ao.render_batch([z for _, z in pairs], params=params), [d for d, _ in pairs], "linear")
    ao.close()
print("mixed ok")
"""


def test_mixed_per_frame_calls_run_ieee_division_for_the_whole_call(tmp_path):
    k = H.kernel_trace(tmp_path, MIXED_CHILD)
    cols = {K.column_of(n) for n in k.short} - {None}
    assert {c for c in cols if c[0] != "ds"} == {("0", "false", "1"), ("1", "false", "1")}, sorted(cols)
    assert {c for c in cols if c[0] == "ds"} == {("ds", "1")}, sorted(cols)
    for family in ("render_small_frames_kernel", "upsample_final_small_frames_kernel", "upsample_final_small_pitched_frames_kernel",
                   "upsample_final_small_linear_frames_kernel", "downsample_frames_kernel", "downsample_pitched_frames_kernel",
                   "downsample_linear_frames_kernel"):
        assert k[family] > 0, (family, sorted(set(k.short)))
    assert not [n for n in k.short if K.split(n)[0].startswith(("render", "upsample")) and "_frames_" not in n], sorted(set(k.short))


# ---- the prefetch reuse key: a pass carried by an IEEE call stamped no hostile flags

def pipelined_calls(oracle, steps, w=384, h=256, n=2):
    """steps: (frames, params or None) per call; call k announces the frames of call k + 1.  Returns the DOWNSAMPLE slot of each
    call, the hostile-frame masks, and checks every output against the oracle under its call's parameters."""
    import torch
    base = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    dd = [[torch.from_numpy(d).to(dev) for d in frames] for frames, _ in steps]
    out = [[torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(n)] for _ in steps]
    st = torch.cuda.current_stream(dev).cuda_stream
    ao = H.component(base, max_batch=n, pipelined=True)
    ds_ms, hostile = [], []
    try:
        for k, (frames, params) in enumerate(steps):
            if k + 1 < len(steps):
                ao.prefetch_device([t.data_ptr() for t in dd[k + 1]], params=steps[k + 1][1])
            ao.set_profiling(True)
            ao.execute_device([t.data_ptr() for t in dd[k]], [t.data_ptr() for t in out[k]], st, params=params)
            ms, execs = ao.pass_times_ms()
            assert execs == 1
            ds_ms.append(ms[PASS_DOWNSAMPLE])
            hostile.append(ao.hostile_frames())
            if k + 1 == len(steps):
                torch.cuda.synchronize(dev)
                sets = [base if params is None else frame_settings(base, p) for p in (params or [None] * n)]
                check_frames(oracle, ao, frames, sets)
        torch.cuda.synchronize(dev)
        for k, (frames, params) in enumerate(steps):
            for f in range(n):
                s = base if params is None else frame_settings(base, params[f])
                got, want = out[k][f].cpu().numpy(), oracle.run(frames[f], s, result_only=True)["result"]
                assert np.array_equal(got, want), (k, f, H.diff_report("result", got, want))
    finally:
        ao.close()
    return ds_ms, hostile


IEEE = [FrameParams(upsampleTolerance=-14.0), FrameParams(upsampleTolerance=-14.0, intensity=2.0)]


def test_pass_carried_by_an_ieee_call_reruns_for_an_exact_call(oracle):
    w, h = 384, 256
    a = [synth.make("S2", w, h, seed=50), synth.make("S2", w, h, seed=51)]
    b = [hostile_level_texels(w, h, 52), synth.make("S2", w, h, seed=53)]
    ds_ms, hostile = pipelined_calls(oracle, [(a, IEEE), (b, None)])
    assert ds_ms[0] > 0
    assert ds_ms[1] > 0, ds_ms              # the carried pass stamped no hostile flags: the exact call re-ran it
    assert hostile[1] == 0b01, hostile


def test_pass_carried_by_an_exact_call_is_reused_by_an_ieee_call(oracle):
    w, h = 384, 256
    a = [synth.make("S2", w, h, seed=60), synth.make("S2", w, h, seed=61)]
    b = [hostile_level_texels(w, h, 62), synth.make("S2", w, h, seed=63)]
    ds_ms, _ = pipelined_calls(oracle, [(a, None), (b, IEEE)])
    assert ds_ms[0] > 0 and ds_ms[1] == 0, ds_ms


def test_pipelined_stream_alternating_columns(oracle):
    w, h = 384, 256
    frames = [[synth.make("S2", w, h, seed=70 + 2 * k), synth.make("S2", w, h, seed=71 + 2 * k)] for k in range(4)]
    frames[2][0] = hostile_level_texels(w, h, 75)
    frames[3][1] = hostile_level_texels(w, h, 76)
    ds_ms, hostile = pipelined_calls(oracle, [(frames[0], None), (frames[1], IEEE), (frames[2], None), (frames[3], IEEE)])
    assert ds_ms[0] > 0 and ds_ms[1] == 0 and ds_ms[2] > 0 and ds_ms[3] == 0, ds_ms
    assert hostile[2] == 0b01, hostile
