"""Coverage gate: every kernel instantiation the library ships is launched and compared with the CPU oracle.

The inventory (tests/kernel_inventory.py) lists the instantiations of the loaded library.  A context runs one column of template
arguments (AOFMT, RTNE, DIV): set by ao_format and f16_rounding, and for RTZ storage by whether the parameters lie in the exact
division range (upsampleTolerance -14 takes the IEEE column).  Each case below runs a child under rocprofv3 --kernel-trace that
drives one column through every launch family and structure the API has -- shared, per-frame, pitched and linear-depth calls,
small and large tiles, nested and separate blends, wide and exhaustive render, a carried composite, the carried downsample of a
pipelined stream -- and checks every frame's result and every valid debug buffer of frame 0 against the oracle, NaN-aware; it
stops at the first mismatch.  The test then asserts that every instantiation of the column was launched."""
import pytest

from tests import helpers as H
from tests import kernel_inventory as K

pytestmark = pytest.mark.gpu

# (AOFMT, RTNE, DIV) of each column, and the settings that select it
COLUMNS = {
    "r8_rtz_exact": (("0", "false", "0"), dict()),
    "r8_rtz_ieee": (("0", "false", "1"), dict(upsample_tolerance=-14.0)),
    "r8_rtne": (("0", "true", "1"), dict(f16_rounding=1)),
    "f16_rtz_exact": (("1", "false", "0"), dict(ao_format=1)),
    "f16_rtz_ieee": (("1", "false", "1"), dict(ao_format=1, upsample_tolerance=-14.0)),
    "f16_rtne": (("1", "true", "1"), dict(ao_format=1, f16_rounding=1)),
}

# instantiations no call of the API launches; each is covered elsewhere
EXCLUDED = {
    "selftest_div_kernel": "meao_selftest only: test_hardware_conversions_exhaustive",
    "selftest_f16_decode_kernel": "meao_selftest only: test_hardware_conversions_exhaustive",
    "selftest_f16_kernel<false>": "meao_selftest only: test_hardware_conversions_exhaustive",
    "selftest_f16_kernel<true>": "meao_selftest only: test_hardware_conversions_exhaustive",
    "selftest_unorm8_decode_kernel": "meao_selftest only: test_hardware_conversions_exhaustive",
}

CHILD = r"""
import dataclasses
import sys
import time

import numpy as np
import torch

from oracle import oracle as O
from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import gpu_kit
from tests import helpers as H
from tests.test_kernel_coverage_gpu import COLUMNS          # the child's own parent module, for this data table alone
from tests.linear_depth import linearize, to_linear

t0 = time.time()
O.build()
CAM = synth.Camera(near=0.1, far=128.0, reversed_z=True)      # far a power of two: linear z = dist * far exactly
DEV = torch.device("cuda", 0)
LIN = linearize()
BIG = 1 << 20
F32, U16, LF32, LF16 = L.DEPTH_F32, L.DEPTH_UNORM16, L.DEPTH_LINEAR_F32, L.DEPTH_LINEAR_F16
NP_DEPTH = {F32: np.float32, U16: np.uint16, LF32: np.float32, LF16: np.float16}
seed = [100]


def compare(what, got, want):
    if not H.nan_aware_equal(got, want)[0]:
        sys.exit("MISMATCH %s: %s" % (what, H.diff_report(what.split()[-1], got, want)))


def frames_for(fmt, w, h, n):
    # (the oracle's raw frames, the library's input frames) of n frames in depth format fmt
    seed[0] += n
    raws = [synth.occluder_field(w, h, seed=seed[0] + f, cam=CAM) for f in range(n)]
    if fmt == F32:
        return raws, raws
    if fmt == U16:
        enc = [O.encode_depth(r, U16) for r in raws]
        return enc, enc
    pairs = [to_linear(LIN, r, CAM) for r in raws]
    return [d for d, _ in pairs], [z.astype(NP_DEPTH[fmt]) for _, z in pairs]


def frame_params(base, n):
    ups = base.upsample_tolerance
    ps = [FrameParams(intensity=1.0 + 0.25 * f, thicknessModifier=1.0 + f, upsampleTolerance=ups - 0.5 * f if ups < -13 else ups + 0.5 * f,
                      blurTolerance=-4.6 + 0.5 * f) for f in range(n)]
    sets = [dataclasses.replace(base, intensity=p.intensity, thickness_modifier=p.thicknessModifier, upsample_tolerance=p.upsampleTolerance,
                                blur_tolerance=p.blurTolerance) for p in ps]
    return ps, sets


def expected(s, fmt, oracle_frames, inputs, params, sets, debug):
    # per frame: dict buffer name -> array.  Linear f16 frames: a linear f32 context run on the widened values (the f16 values are
    # not the Linearize of a raw frame); that context's own kernels are the LINEAR_F32 ones, compared with the oracle elsewhere here.
    if fmt != LF16:
        return [O.run(d, dataclasses.replace(sf, depth_format=U16 if fmt == U16 else F32), nthreads=8, result_only=f > 0)
                for f, (d, sf) in enumerate(zip(oracle_frames, sets))]
    ref = H.component(s, max_batch=len(inputs), depth_format=LF32, debug=debug)
    try:
        outs = ref.render_batch([z.astype(np.float32) for z in inputs], params=params)
        res = [{"result": o} for o in outs]
        for i in H.valid_debug_ids(s.num_levels, s.hq_levels):
            res[0][H.NAMES[i]] = ref.debug_buffer(i)
        return res
    finally:
        ref.close()


def device_frames(arrs, pitch):
    # one allocation holding the frames as surfaces of `pitch` elements per row, the padding zero: (surface, pointers, pitch in bytes)
    (h, w) = arrs[0].shape
    s = gpu_kit.Surface(w, h, arrs[0].dtype, n=len(arrs), pitch=pitch, fill=0, content=arrs, device=DEV)
    return s, s.ptrs(), s.row_bytes


def read_frames(what, s):
    raw = s.download()
    if not s.intact(raw):
        sys.exit("MISMATCH %s: row padding was written" % what)
    return [s.texels(f, raw) for f in range(s.n)]


def check(what, ao, s, outs, want):
    for f, o in enumerate(outs):
        compare("%s frame %d result" % (what, f), o, want[f]["result"])
    for i in H.valid_debug_ids(s.num_levels, s.hq_levels):
        compare("%s frame 0 %s" % (what, H.NAMES[i]), ao.debug_buffer(i, frame=0), want[0][H.NAMES[i]])


def run(w, h, n, fmt=F32, debug=None, per_frame=False, pitch=0, steps=0, composite=False, **cfg):
    # one configuration: a host call, or device frames (pitch: row pitch in elements, 0 = packed), or a pipelined stream of
    # `steps` device calls, each announcing the next one's frames
    s = dataclasses.replace(H.settings(O, w, h, cam=CAM), **COLUMNS[sys.argv[1]][1], **cfg)
    what = "%dx%d n=%d fmt=%d debug=%s per_frame=%s pitch=%d steps=%d composite=%s %s" % (w, h, n, fmt, debug, per_frame, pitch, steps,
                                                                                          composite, cfg)
    ao = H.component(s, max_batch=n, debug=debug, depth_format=fmt, pipelined=steps > 0)
    ao_dt = np.uint8 if s.ao_format == L.AO_R8 else np.uint16
    try:
        calls = []
        for k in range(max(steps, 2 if composite else 1)):
            oracle_frames, inputs = frames_for(fmt, w, h, n)
            params, sets = frame_params(s, n) if per_frame else (None, [s] * n)
            calls.append((oracle_frames, inputs, params, sets))
        if not (pitch or steps or composite):
            oracle_frames, inputs, params, sets = calls[0]
            outs = ao.render_batch(inputs, params=params)
            check(what, ao, s, outs, expected(s, fmt, oracle_frames, inputs, params, sets, debug))
            return
        dp = pitch or w
        st = torch.cuda.current_stream(DEV).cuda_stream
        dev_in = [device_frames(c[1], dp) for c in calls]
        dev_out = [device_frames([np.zeros((h, w), ao_dt)] * n, dp) for _ in calls]
        pitches = dict(depth_pitch=dev_in[0][2], out_pitch=dev_out[0][2]) if pitch else {}
        for k, (oracle_frames, inputs, params, sets) in enumerate(calls):
            if steps and k + 1 < steps:
                ao.prefetch_device(dev_in[k + 1][1], params=calls[k + 1][2], depth_pitch=pitches.get("depth_pitch", 0))
            if composite and k == 1:
                colors = [np.random.default_rng(f).uniform(0, 2, (h, w, 4)).astype(np.float16).view(np.uint16) for f in range(n)]
                col = [torch.from_numpy(c.view(np.int16).copy()).to(DEV) for c in colors]
                ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, dev_out[0][1], [c.data_ptr() for c in col])
            ao.execute_device(dev_in[k][1], dev_out[k][1], st, params=params, **pitches)
        torch.cuda.synchronize(DEV)
        for k, (oracle_frames, inputs, params, sets) in enumerate(calls):
            outs = read_frames(what, dev_out[k][0])
            want = expected(s, fmt, oracle_frames, inputs, params, sets, debug) if k + 1 == len(calls) else \
                [{"result": r["result"]} for r in expected(s, fmt, oracle_frames, inputs, params, sets, debug)]
            if k + 1 == len(calls):
                check(what + " call %d" % k, ao, s, outs, want)
            else:
                for f, o in enumerate(outs):
                    compare("%s call %d frame %d result" % (what, k, f), o, want[f]["result"])
        if composite:
            first = read_frames(what, dev_out[0][0])
            for f in range(n):
                want_col = colors[f].copy()
                O.composite(np.ascontiguousarray(first[f]), want_col, 0, ao_format=s.ao_format)
                compare("%s composite frame %d color" % (what, f), col[f].cpu().numpy().view(np.uint16), want_col)
    finally:
        ao.close()


NO_SMALL = {L.DEBUG_RENDER_SMALL_MAX_TILES: 0, L.DEBUG_FINAL_SMALL_MAX_TILES: 0, L.DEBUG_DS_SMALL_MAX_TILES: 0}
BIG_SMALL = {L.DEBUG_RENDER_SMALL_MAX_TILES: BIG, L.DEBUG_FINAL_SMALL_MAX_TILES: BIG, L.DEBUG_DS_SMALL_MAX_TILES: BIG}
TWO_LEVEL = {L.DEBUG_NESTED_MAX_TILES: 0, L.DEBUG_BLEND_TALL_MIN_TILES: 0}
TALL = {L.DEBUG_NESTED_MAX_TILES: 0, L.DEBUG_BLEND_TALL_MIN_TILES: 1}
SEPARATE = {L.DEBUG_FUSE_COARSE_BLEND: 0}

for per_frame in (False, True):
    # raw f32 / unorm16 frames, packed: every render and blend structure, both final tile heights, both downsample row counts;
    # W % 8 != 0 takes the scalar downsample
    run(384, 256, 2, per_frame=per_frame, debug={L.DEBUG_NESTED_MAX_TILES: BIG, **BIG_SMALL})
    run(384, 256, 3, per_frame=per_frame, debug={**TWO_LEVEL, **NO_SMALL})
    run(380, 250, 1, per_frame=per_frame, debug=TALL)
    run(380, 250, 2, per_frame=per_frame, debug={**SEPARATE, **NO_SMALL})
    run(376, 248, 6, per_frame=per_frame, debug={**SEPARATE, **BIG_SMALL})
    run(384, 256, 1, per_frame=per_frame, sample_set=L.SAMPLES_EXHAUSTIVE)
    run(384, 256, 2, per_frame=per_frame, hq_levels=2)
    run(200, 120, 1, per_frame=per_frame, hq_levels=2, sample_set=L.SAMPLES_EXHAUSTIVE)
    run(384, 256, 2, U16, per_frame=per_frame, debug=BIG_SMALL)
    run(380, 250, 2, U16, per_frame=per_frame, debug=NO_SMALL)
    # pipelined streams: the next batch's pass carried in the last kernel (f32, W % 8 == 0), or as its own launch
    run(384, 256, 2, per_frame=per_frame, steps=3)
    run(384, 256, 2, per_frame=per_frame, steps=3, debug={L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: 1})
    # pitched surfaces: vector (pitch % 4 == 0) and scalar rows, both tile heights, f32 and unorm16, carried pass
    run(384, 256, 2, per_frame=per_frame, pitch=392, debug=BIG_SMALL)
    run(384, 256, 2, per_frame=per_frame, pitch=392, debug=NO_SMALL)
    run(384, 256, 2, per_frame=per_frame, pitch=389, debug=BIG_SMALL)
    run(384, 256, 2, per_frame=per_frame, pitch=389, debug=NO_SMALL)
    run(384, 256, 2, U16, per_frame=per_frame, pitch=392, debug=BIG_SMALL)
    run(384, 256, 2, U16, per_frame=per_frame, pitch=392, debug=NO_SMALL)
    run(384, 256, 2, per_frame=per_frame, pitch=392, steps=3)
    # linear view-space depth, f32 and f16, packed and pitched, carried pass
    for fmt in (LF32, LF16):
        run(384, 256, 2, fmt, per_frame=per_frame, debug=BIG_SMALL)
        run(384, 256, 2, fmt, per_frame=per_frame, debug=NO_SMALL)
        run(380, 250, 2, fmt, per_frame=per_frame, debug=BIG_SMALL)
        run(380, 250, 2, fmt, per_frame=per_frame, debug=NO_SMALL)
        run(384, 256, 2, fmt, per_frame=per_frame, pitch=392, debug=NO_SMALL)
    run(384, 256, 2, LF32, per_frame=per_frame, steps=3)
# a composite enqueued behind a call rides in the next shared call's render kernel
run(384, 256, 2, composite=True)
print("coverage child %s ok: %.1f s" % (sys.argv[1], time.time() - t0))
"""

INDEPENDENT_CHILD = r"""
import sys
import time


import numpy as np

from oracle import oracle as O
from miniengineao_amd import synth
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests.linear_depth import linearize, to_linear

t0 = time.time()
O.build()
LIN = linearize()
w, h = 96, 64
for ao_format in (L.AO_R8, L.AO_F16):
    for rounding in (L.F16_RTZ_CLAMP, L.F16_RTNE):
        s = H.settings(O, w, h, ao_format=ao_format, f16_rounding=rounding)
        d = synth.make("S2", w, h, seed=3)
        want = O.run(d, s)
        with H.component(s) as ao:
            got = ao.render(d)
            for i in (1, 6, 7, 8, 9):                  # LinearDepth and TiledDepth1..4, built on demand
                if not H.nan_aware_equal(ao.debug_buffer(i), want[H.NAMES[i]])[0]:
                    sys.exit("MISMATCH %d %d id %d: %s" % (ao_format, rounding, i, H.diff_report(H.NAMES[i], ao.debug_buffer(i), want[H.NAMES[i]])))
            for i in (1, 3, 7, 11, 15, 17):            # debug views
                v, wv = ao.debug_view(i), O.debug_view(want, i, s)
                if not np.array_equal(v, wv):
                    sys.exit("MISMATCH %d %d view %d: %s" % (ao_format, rounding, i, H.diff_report("view", v, wv)))
            color = np.random.default_rng(4).uniform(0, 2, (h, w, 4)).astype(np.float16).view(np.uint16)
            want_col = color.copy()
            O.composite(np.ascontiguousarray(want["result"]), want_col, 0, ao_format=ao_format)
            ao.composite(got, color)
            if not np.array_equal(color, want_col):
                sys.exit("MISMATCH composite %d: %s" % (ao_format, H.diff_report("color", color, want_col)))
        cam = synth.Camera(near=0.1, far=128.0, reversed_z=True)
        sl = H.settings(O, w, h, cam=cam, ao_format=ao_format, f16_rounding=rounding)
        raw, z = to_linear(LIN, synth.occluder_field(w, h, seed=5, cam=cam), cam)
        with H.component(sl, depth_format=L.DEPTH_LINEAR_F32) as ao:      # LinearDepth of linear frames
            ao.render(z)
            got1, want1 = ao.debug_buffer(1), O.run(raw, sl)["linear_depth"]
            if not H.nan_aware_equal(got1, want1)[0]:
                sys.exit("MISMATCH linear depth view %d: %s" % (rounding, H.diff_report("linear_depth", got1, want1)))
print("coverage child independent ok: %.1f s" % (time.time() - t0))
"""


def column_entries(col):
    return {n for n in K.instantiations() if K.column_of(n) in (col, ("ds", col[2]))}


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_instantiation_of_the_column_launched_and_exact(tmp_path, name):
    col, _ = COLUMNS[name]
    k = H.kernel_trace(tmp_path, CHILD, [name])
    print(k.stdout.strip().splitlines()[-1])
    launched = set(k.short)
    missing = sorted(column_entries(col) - launched)
    assert not missing, "%d of %d instantiations of column %s never launched: %s" % (len(missing), len(column_entries(col)), name, missing)
    stray = sorted(n for n in launched if K.column_of(n) and K.column_of(n)[0] != "ds" and K.column_of(n) != col)
    assert not stray, stray


def test_every_column_independent_instantiation_launched_and_exact(tmp_path):
    k = H.kernel_trace(tmp_path, INDEPENDENT_CHILD)
    print(k.stdout.strip().splitlines()[-1])
    want = {n for n in K.instantiations() if K.column_of(n) is None}
    assert set(EXCLUDED) <= want, sorted(set(EXCLUDED) - want)
    missing = sorted(want - set(EXCLUDED) - set(k.short))
    assert not missing, missing
