"""The dynamic-resolution suite's frames, surfaces and pipelined Stream (tests/test_dynamic_resolution_gpu.py and
tests/dynamic_resolution_testhooks_check.py): a reservation of 400 x 272 and the sizes inside it."""
import numpy as np

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from tests import gpu_kit
from tests import helpers as H

RES = (400, 272)
LADDER = [(384, 256), (200, 120), (380, 250), (97, 61), (33, 17), (400, 272), (200, 120)]
GUARD = 256                           # sentinel bytes in front of and behind every surface

_frames = {}


def frame(kind, w, h, seed):
    """Distinct contents: "S2" = synth.make("S2"), "field" = a sparser synth.occluder_field."""
    key = (kind, w, h, seed)
    if key not in _frames:
        _frames[key] = synth.make("S2", w, h, seed=seed) if kind == "S2" else synth.occluder_field(w, h, seed=seed, n_rects=48, n_discs=24)
    return _frames[key]


def call_frames(k, w, h):
    """The two frames of call k: an S2 frame and an occluder field, other contents in every call."""
    return [frame("S2", w, h, 3 + 2 * k), frame("field", w, h, 1000 + 7 * k)]


def want_of(oracle, depth, s, key, full=False):
    """The oracle's buffers for `depth` under `s`, computed once per (frame, settings)."""
    return H.want_of(oracle, key, depth, s, result_only=not full)


class Surfaces:
    """n device surfaces of surf = (sw, sh) texels of `dtype`, one allocation each, filled with a pattern, the frames (size = (w, h))
    in their top-left viewports."""

    def __init__(self, n, surf, size, dtype, tail=(), frames=None):
        self.each = [gpu_kit.Surface(size[0], size[1], dtype, tail, pitch=surf[0], rows=surf[1], guard=GUARD,
                                     content=None if frames is None else [frames[f]]) for f in range(n)]
        self.pitch = self.each[0].row_bytes

    def ptrs(self):
        return [s.ptr for s in self.each]

    def get(self, f):
        """(the viewport of surface f, whether every byte outside it still holds what the host put there)"""
        return self.each[f].read()


PER_FRAME = [dict(), dict(intensity=1.5, thickness_modifier=2.0)]       # frame 1 of a per-frame call has parameters of its own


class Stream:
    """A pipelined context with a reservation, fed depth frames in 400 x 272 surfaces or packed.  Shared parameters: the camera
    does not change with the size (one proj00, the oracle's Settings take it: meao_set_params would drop every announcement);
    per-frame parameters: every frame brings the proj00 of its size, as H.settings computes it."""

    def __init__(self, torch, oracle, own_launch, per_frame, first):
        self.torch, self.O, self.per_frame = torch, oracle, per_frame
        self.proj00 = H.settings(oracle, *first).proj00
        self.ao = H.component(self.settings(*first), max_batch=2, pipelined=True, debug={L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: own_launch})
        self.ao.reserve(*RES)
        self.ao.set_profiling(True)
        self.keep = []

    def settings(self, w, h, f=0):
        s = H.settings(self.O, w, h, **(PER_FRAME[f] if self.per_frame else {}))
        if not self.per_frame:
            s.proj00 = self.proj00
        return s

    def params(self, w, h):
        if not self.per_frame:
            return None
        return [FrameParams(intensity=s.intensity, thicknessModifier=s.thickness_modifier, projection00=s.proj00)
                for s in (self.settings(w, h, f) for f in range(2))]

    def batch(self, k, w, h):
        """Device frames of step k (packed) and the AO surfaces they will be written to."""
        raw = call_frames(k, w, h)
        din = Surfaces(2, (w, h), (w, h), np.float32, frames=raw)
        out = Surfaces(2, (w, h), (w, h), np.uint8)
        self.keep.append((din, out))
        return dict(k=k, size=(w, h), raw=raw, din=din, out=out)

    def announce(self, b, sized=True):
        self.ao.prefetch_device(b["din"].ptrs(), self.params(*b["size"]), size=b["size"] if sized else None)

    def execute(self, b):
        self.ao.execute_device(b["din"].ptrs(), b["out"].ptrs(), params=self.params(*b["size"]))

    def check(self, b):
        self.ao.synchronize()
        w, h = b["size"]
        for f in range(2):
            want = want_of(self.O, b["raw"][f], self.settings(w, h, f), (b["k"], f))["result"]
            got, _ = b["out"].get(f)
            assert np.array_equal(got, want), (b["k"], b["size"], f, H.diff_report("result", got, want))

    def downsample_ms(self, b):
        """The DOWNSAMPLE slot of executing `b` alone: 0 = that call launched no downsample pass."""
        ms = H.downsample_ms(self.ao, lambda: self.execute(b))
        self.check(b)
        return ms


A, B, C3 = (384, 256), (200, 120), (380, 250)
