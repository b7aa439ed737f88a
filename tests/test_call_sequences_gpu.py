"""Long call sequences on one long-lived context and on the pool, against a model of the host-visible state.

tests/call_model.py predicts, from include/meao.h alone, what every call must do given everything before it: whether its own
downsample pass runs or a prefetched one is reused, whether it carries an announced pass, whether a waiting composite rides or
runs as plain launches.  The Driver below issues the same operations to the real library.  Stepped mode synchronises after every
operation and compares everything that can be observed (results against the CPU oracle, every byte of the surfaces passed, the pass
times, the composite state, the hostile mask, debug buffers); free-running mode submits the whole sequence without waiting and
counts launches by kernel name in a rocprofv3 trace.  Everything a free-running sequence will copy into its buffers (depth frames,
colour targets) is put on the device before the first call and copied from there in stream order.  The one exception is the pool:
its members' streams are its own, so a buffer is filled (once, before its first use) and a colour target reset by a blocking copy
from host memory -- which waits for none of the members' non-blocking streams, so nothing the pool has in flight is held up.

An execute has a size, two row strides and oracle settings PER FRAME (Driver.geometry): the context's size under the call's
pitches for every call but meao_execute_batch_extents (Op.extents; tests/test_mixed_size_sequences_gpu.py draws those).

Every surface of a sequence has the size of the largest frame plus the widest pitch and stays allocated until the sequence has
ended, so that a call running on stale bookkeeping still reads and writes live memory of the right size.
"""
import ctypes as C
import contextlib
import dataclasses
import json
import random
import re
import time

import numpy as np
import pytest

from miniengineao_amd import FrameParams, synth
from miniengineao_amd import _lib as L
from miniengineao_amd.frame_params import params_array, to_params
from tests import call_model as M
from tests import helpers as H
from tests.helpers import PASS_DOWNSAMPLE, downsample_ms

pytestmark = pytest.mark.gpu

CAM_LINEAR = synth.Camera(near=0.1, far=128.0, reversed_z=True)       # palette entries M.LINEAR_TAGS
DEPTH_FORMATS = {"f32": (L.DEPTH_F32, np.float32), "unorm16": (L.DEPTH_UNORM16, np.uint16), "linear_f32": (L.DEPTH_LINEAR_F32, np.float32)}
PATTERN = 0xA5


def fields_of(tag, w, h):
    """Palette entry `tag` as oracle Settings fields (proj00 for a w x h frame)."""
    f = M.PALETTE_FIELDS[tag]
    cam = synth.Camera(f["near"], f["far"], f["fov"], f["rev"])
    return dict(near_clip=f["near"], far_clip=f["far"], reversed_z=f["rev"], proj00=cam.proj00(w, h), intensity=f["intensity"],
                thickness_modifier=f["thickness"], noise_filter_tolerance=f["noise"], blur_tolerance=f["blur"],
                upsample_tolerance=f["upsample"])


def frame_params_of(fields):
    return FrameParams(nearClipPlane=fields["near_clip"], farClipPlane=fields["far_clip"], projection00=fields["proj00"],
                       usesReversedZBuffer=fields["reversed_z"], singlePassStereoEnabled=False, intensity=fields["intensity"],
                       thicknessModifier=fields["thickness_modifier"], noiseFilterTolerance=fields["noise_filter_tolerance"],
                       blurTolerance=fields["blur_tolerance"], upsampleTolerance=fields["upsample_tolerance"])


class Surface:
    """A device allocation of full size with a host mirror of every byte the device must hold.  oracle_bytes: what the oracle reads
    for the same texels (differs from the mirror for linear depth only: the raw frame whose Linearize the device frame is)."""

    def __init__(self, torch, dev, nbytes, fill):
        self.mirror = np.full(nbytes, fill, np.uint8)
        self.oracle_bytes = self.mirror
        self.dev = torch.from_numpy(self.mirror).to(dev)

    def ptr(self):
        return self.dev.data_ptr()

    @staticmethod
    def view(raw, dtype, pitch, w, h):
        e = np.dtype(dtype).itemsize
        return raw[:h * pitch * e].view(dtype).reshape(h, pitch)[:, :w]


class Driver:
    def __init__(self, oracle, cfg, profile, own_launch, lin_c=None, stepped=True, seed=0):
        import torch
        self.torch, self.O, self.cfg, self.P, self.stepped, self.lin_c = torch, oracle, cfg, profile, stepped, lin_c
        self.own_launch = own_launch
        self.rng = random.Random(seed)
        self.dev = torch.device("cuda", 0)
        self.G = profile.pool
        self.w, self.h = profile.sizes[0]
        self.fmt, self.depth_dt = DEPTH_FORMATS[cfg.get("depth", "f32")]
        self.linear = cfg.get("linear", False)
        self.ao_fmt = L.AO_F16 if cfg.get("ao") == "f16" else L.AO_R8
        self.ao_dt = np.uint16 if self.ao_fmt == L.AO_F16 else np.uint8
        self.rounding = L.F16_RTZ_CLAMP if cfg.get("rtz", True) else L.F16_RTNE
        self.hq = cfg.get("hq_levels", 0)
        frames = profile.sizes + profile.outside_sizes + profile.mixed_sizes      # every size a frame of the sequence can have
        wmax, hmax = max(s[0] for s in frames), max(s[1] for s in frames)
        if profile.mixed_sizes:                              # (and the extents of the mixed calls the library must refuse)
            wmax, hmax = wmax + 16, hmax + 8
        self.cap = hmax * max(wmax + max(M.PITCH_EXTRA), M.PITCH_FIXED)      # texels of every surface
        self.lib = L.load()
        self.ctx_fields = fields_of(0, self.w, self.h)
        base = self.settings(self.ctx_fields)
        if self.G:
            from miniengineao_amd import AmbientOcclusionPool
            self.ao = AmbientOcclusionPool(self.w, self.h, [0] * self.G, max_batch=profile.max_batch, ao_format=self.ao_fmt,
                                           pipelined=cfg.get("pipelined", True), depth_format=self.fmt)
            self.base_prm = self.ao._prm
            self.apply_params(self.ctx_fields)
            self.members = [self.ao.member_context(m) for m in range(self.G)]
            for c in self.members:
                L.check(self.lib.meao_debug_set(c, L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH, own_launch), c)
            self.streams = [None]
        else:
            self.ao = H.component(base, max_batch=profile.max_batch, debug={L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: own_launch},
                                  depth_format=self.fmt, pipelined=cfg.get("pipelined", True))
            self.ao._sync_params()
            self.base_prm = self.ao._prm
            self.members = [self.ao._ctx]
            self.streams = [torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)]
        self.cur = 0
        de, ae = np.dtype(self.depth_dt).itemsize, np.dtype(self.ao_dt).itemsize
        self.depth = {}
        self.outs = {}
        self.colors = {}
        self.depth_bytes, self.out_bytes = self.cap * de, self.cap * ae
        self.frames = {}
        self.oracle_cache = {}
        self.library = {}            # free-running: device copies of what the refills will write
        self.color_want = {}         # colour id -> what it must hold once its composite has run
        self.color_lib = {}
        self.checks = []             # free-running: the AO surfaces to compare at the end
        self.viewed = False
        self.laid = {}               # depth buffer -> (content key, (pitch, w, h) it was laid out with)
        self.final_color = {}        # free-running: colour id -> what it must hold at the end
        self.bg = None
        self.last_read = None        # the last execute: (op, [(oracle frame, fields)], expects), for reads some operations later
        self.log = []
        self.fusable = 0             # carried passes that the header allows inside the carrier's last kernel (see note_fusable)

    # ---- settings, parameters
    def settings(self, fields, w=None, h=None):
        return self.O.Settings(w or self.w, h or self.h, ao_format=self.ao_fmt, f16_rounding=self.rounding, hq_levels=self.hq,
                               depth_format=L.DEPTH_F32 if self.linear else self.fmt, **fields)

    def fields_for(self, param):
        return fields_of(param.tag, self.w, self.h)

    def apply_params(self, fields):
        p = to_params(frame_params_of(fields), self.base_prm)
        if self.G:
            self.ao._check(self.lib.meao_pool_set_params(self.ao._pool, C.byref(p)))
        else:
            L.check(self.lib.meao_set_params(self.ao._ctx, C.byref(p)), self.ao._ctx)
        self.ctx_fields = fields

    def params_ctypes(self, params):
        fps = []
        for p in params:
            f = self.fields_for(p)
            fps.append(frame_params_of(f))
        return params_array(fps, len(fps), self.base_prm)

    # ---- surfaces and contents
    def surface(self, table, i, nbytes, fill):
        if i not in table:
            table[i] = Surface(self.torch, self.dev, nbytes, fill)
        return table[i]

    def depth_surface(self, i):
        if i not in self.depth:
            s = self.depth[i] = Surface(self.torch, self.dev, self.depth_bytes, 0)
            dev_bg, oracle_bg = self.background()
            s.mirror[:] = dev_bg
            if self.linear:
                s.oracle_bytes = oracle_bg.copy()
            s.dev.copy_(self.torch.from_numpy(s.mirror))
        return self.depth[i]

    def background(self):
        """What a depth surface holds outside the frames laid out in it: a valid depth everywhere (bytes for the device, for the oracle)."""
        if self.bg is None:
            half = np.full(self.cap, 0.5 if self.fmt != L.DEPTH_UNORM16 else 0x8000, self.depth_dt)
            if self.linear:
                d, z = self.to_linear(half.reshape(1, -1))
                self.bg = (z.reshape(-1).view(np.uint8).copy(), d.reshape(-1).view(np.uint8).copy())
            else:
                self.bg = (half.view(np.uint8).copy(), half.view(np.uint8).copy())
        return self.bg

    def to_linear(self, d):
        from tests.linear_depth import to_linear
        return to_linear(self.lin_c, d, CAM_LINEAR)

    def frame(self, content, w, h):
        """(device frame, oracle frame) of a content key at w x h, in the depth format of the case."""
        key = (content, w, h)
        if key not in self.frames:
            kind, seed = content
            if kind == "synth" or self.fmt == L.DEPTH_UNORM16:      # UNORM codes cannot be hostile: another clean frame
                d = synth.make("S2", w, h, seed=40 + seed + (100 if kind != "synth" else 0))
            elif kind == "hostile":
                d = H.hostile_frame(w, h, 60 + seed)
            else:
                from tests.helpers import hostile_level_texels
                d = hostile_level_texels(w, h, 80 + seed)
                if w * h < 200 * 120:
                    # a few hundred texels (the small frames of a mixed call): the sprinkled ones may miss the texels the levels
                    # are made of, so one of every hostile kind is planted there (y and x even) -- the bit is known again
                    for i, v in enumerate(H.hostile_values().values()):
                        d[2 * (i // 4), 2 * (i % 4)] = v
            d = np.ascontiguousarray(d, np.float32)
            if self.fmt == L.DEPTH_UNORM16:
                d = np.round(np.clip(d, 0, 1) * 65535).astype(np.uint16)
                self.frames[key] = (d, d)
            elif self.linear:
                raw, z = self.to_linear(d)
                self.frames[key] = (z, raw)
            else:
                self.frames[key] = (d, d)
        return self.frames[key]

    def stream_handle(self):
        return self.streams[self.cur].cuda_stream if not self.G else 0

    def on_stream(self):
        return self.torch.cuda.stream(self.streams[self.cur]) if not self.G else contextlib.nullcontext()

    def upload(self, surf, lib_key=None):
        if self.stepped or self.G or lib_key is None:
            surf.dev.copy_(self.torch.from_numpy(surf.mirror))        # pageable host memory: returns when the copy is done
        else:
            with self.on_stream():
                surf.dev.copy_(self.library[lib_key], non_blocking=True)

    def prepare(self, ops):
        """Free-running: everything the sequence will copy into its buffers goes to the device first."""
        if self.stepped or self.G:
            return
        size = (self.w, self.h)                                       # the context's, as the sequence will have made it by then
        for op in ops:
            if op.kind == "refill":
                for c in op.contents:
                    key = (c, op.pitch, op.size or size)
                    if key not in self.library:
                        w, h = key[2]
                        img = self.background()[0].copy()
                        self.lay_out(img, self.frame(c, w, h)[0], M.row_texels(op.pitch, w))
                        self.library[key] = self.torch.from_numpy(img).to(self.dev)
            elif op.kind == "resize":
                size = op.size
            elif op.kind == "comp_enqueue":
                for c in op.colors:
                    if c not in self.colors:
                        s = self.surface(self.colors, c, self.cap * 8, 0)
                    if ("color", c, size) not in self.library:
                        base = self.color0(c, *size)
                        img = np.zeros(self.cap * 8, np.uint8)
                        img[:base.nbytes] = base.reshape(-1).view(np.uint8)
                        self.library[("color", c, size)] = self.torch.from_numpy(img).to(self.dev)
        self.torch.cuda.synchronize(self.dev)

    def lay_out(self, raw, frame, pitch):
        h, w = frame.shape
        Surface.view(raw, frame.dtype, pitch, w, h)[:] = frame

    def refill(self, op):
        w, h = op.size or (self.w, self.h)                             # a frame of the size it will be announced at
        pitch = M.row_texels(op.pitch, w)
        for b, c in zip(op.bufs, op.contents):
            s = self.depth_surface(b)
            dev_frame, oracle_frame = self.frame(c, w, h)
            if not self.stepped and not self.G:                        # the library image is the whole surface
                s.mirror[:] = self.background()[0]
                if self.linear:
                    s.oracle_bytes[:] = self.background()[1]
            self.laid[b] = (c, (pitch, w, h))
            self.lay_out(s.mirror, dev_frame, pitch)
            if self.linear:
                self.lay_out(s.oracle_bytes, oracle_frame, pitch)
            self.upload(s, (c, op.pitch, (w, h)))

    def color0(self, i, w=None, h=None):
        w, h = w or self.w, h or self.h
        key = (i, w, h)
        if key not in self.color_lib:
            rng = np.random.default_rng(1000 + i)
            self.color_lib[key] = (rng.random((h, w, 4)) * 2.0).astype(np.float16).view(np.uint16)
        return self.color_lib[key]

    # ---- the oracle
    def want(self, frame, fields, full=False):
        key = (frame.tobytes(), tuple(sorted(fields.items())), frame.shape)
        hit = self.oracle_cache.get(key)
        if hit is None or (full and len(hit) == 1):
            s = self.settings(fields, frame.shape[1], frame.shape[0])
            hit = self.oracle_cache[key] = self.O.run(np.ascontiguousarray(frame), s, result_only=not full)
        return hit

    # ---- operations
    def sync(self):
        if self.G:
            self.ao.synchronize()
        self.torch.cuda.synchronize(self.dev)

    def switch_stream(self, to):
        if not self.G and to != self.cur:
            self.streams[to].wait_stream(self.streams[self.cur])      # a change of stream is ordered by an event wait
            self.cur = to

    def member_expects(self, e):
        return e if isinstance(e, list) else [e]

    def pending(self):
        n = C.c_int32()
        if self.G:
            self.ao._check(self.lib.meao_pool_composite_pending(self.ao._pool, C.byref(n)))
        else:
            L.check(self.lib.meao_composite_pending(self.ao._ctx, C.byref(n)), self.ao._ctx)
        return n.value

    def check_composites(self, op, expects):
        ran = [e.comp_ran for e in expects if e is not None and e.comp_ran is not None]
        for comp in ran:
            if not self.G and comp.stream != self.cur and not self.stepped:
                self.streams[self.cur].wait_stream(self.streams[comp.stream])
            for c in comp.color:
                if self.stepped:
                    self.sync()
                    self.compare_color(c, op)
                else:
                    self.final_color[c] = self.color_want.pop(c)
        if self.stepped:
            models = self.model.members if self.G else [self.model]       # (a member that sat the call out still holds its share)
            want = sum(len(m.comp.ao) for m in models if m.comp is not None)
            assert self.pending() == want, (op, "composite_pending", self.pending(), want)

    def compare_color(self, c, op):
        want = self.color_want.pop(c)
        got = self.colors[c].dev.cpu().numpy()[:want.nbytes].view(np.uint16).reshape(want.shape)
        assert np.array_equal(got, want), (op, "composite of colour %d" % c, H.diff_report("color", got, want))

    def geometry(self, op):
        """[(width, height, depth row stride, AO row stride)] of an execute's frames, in texels: every frame at the context's
        size under the call's pitches, or each at its own (Op.extents)."""
        if op.extents is not None:
            return [(w, h, M.row_texels(dp, w), M.row_texels(ap, w)) for w, h, dp, ap in op.extents]
        return [(self.w, self.h, self.w if op.depth_host else M.row_texels(op.pitch, self.w),
                 self.w if op.out_host else M.row_texels(op.out_pitch, self.w))] * len(op.bufs)

    def is_mixed(self, op):
        """A mixed call: extents that are not all the context's size under one pair of strides."""
        geo = self.geometry(op)
        return op.extents is not None and not (all(g[:2] == (self.w, self.h) for g in geo) and len(set(geo)) == 1)

    def extents_ctypes(self, op, bad=None):
        """The meao_extent array of an execute.  The packed row is given as 0 for even frames and in bytes for odd ones: the
        same stride."""
        de, ae = np.dtype(self.depth_dt).itemsize, np.dtype(self.ao_dt).itemsize
        ext = (L.Extent * max(1, len(op.extents)))()
        for f, (w, h, dp, ap) in enumerate(op.extents):
            ext[f].width, ext[f].height = w, h
            ext[f].depth_pitch = M.row_texels(dp, w) * de if dp or f % 2 else 0
            ext[f].ao_pitch = M.row_texels(ap, w) * ae if ap or f % 2 else 0
        if bad == "extent_pitch_below_row":                           # one texel short of the row of ITS frame
            if op.key == 0:
                ext[op.value].depth_pitch = (op.extents[op.value][0] - 1) * de
            else:
                ext[op.value].ao_pitch = (op.extents[op.value][0] - 1) * ae
        return ext

    def call_execute(self, op, bad=None):
        """meao_execute_batch / _params / _pitched / _extents (or the pool's) as the operation asks; returns the status."""
        n_real = len(op.bufs)
        de, ae = np.dtype(self.depth_dt).itemsize, np.dtype(self.ao_dt).itemsize
        dp = (M.row_texels(op.pitch, self.w)) * de if op.pitch else 0
        opitch = (M.row_texels(op.out_pitch, self.w)) * ae if op.out_pitch else 0
        self.host_out = []
        din, dout = [], []
        for b in op.bufs:
            s = self.depth_surface(b)
            din.append(s.mirror.ctypes.data if op.depth_host else s.ptr())
        for o in op.outs:
            s = self.surface(self.outs, o, self.out_bytes, PATTERN)
            if op.out_host:
                self.host_out.append(s.mirror.copy())
                dout.append(self.host_out[-1].ctypes.data)
            else:
                dout.append(s.ptr())
        prm = None if op.params is None else self.params_ctypes(op.params)
        if bad == "bad_pitch":
            dp = self.w * de - de
        if bad == "null_pointer":
            din[0] = None
        if bad == "n_zero":
            n_real = 0
        if bad == "n_over":
            n_real = self.P.max_batch * (self.G or 1) + 1
            din, dout = (din * n_real)[:n_real], (dout * n_real)[:n_real]
        if bad == "bad_params":
            prm = self.params_ctypes(op.params)
        if op.extents is not None:
            n_real = len(op.extents)                                  # (extent_n_over: one more than the limit)
            din, dout = (din * n_real)[:n_real], (dout * n_real)[:n_real]
            pin, pout = (C.c_void_p * n_real)(*din), (C.c_void_p * n_real)(*dout)
            ext = self.extents_ctypes(op, bad)
            if self.G:
                return self.lib.meao_pool_execute_batch_extents(self.ao._pool, n_real, pin, pout, ext, prm)
            return self.lib.meao_execute_batch_extents(self.ao._ctx, n_real, pin, pout, ext, prm, C.c_void_p(self.stream_handle()))
        k = max(1, len(din))
        pin, pout = (C.c_void_p * k)(*din), (C.c_void_p * k)(*dout)
        dl, ol = (L.MEM_HOST if op.depth_host else L.MEM_DEVICE), (L.MEM_HOST if op.out_host else L.MEM_DEVICE)
        if self.G:
            p = self.ao._pool
            if dp or opitch:
                return self.lib.meao_pool_execute_batch_pitched(p, n_real, pin, dp, dl, pout, opitch, ol, prm)
            if prm is None:
                return self.lib.meao_pool_execute_batch(p, n_real, pin, dl, pout, ol)
            return self.lib.meao_pool_execute_batch_params(p, n_real, pin, dl, pout, ol, prm)
        ctx, st = self.ao._ctx, C.c_void_p(self.stream_handle())
        if dp or opitch or bad == "bad_pitch":
            return self.lib.meao_execute_batch_pitched(ctx, n_real, pin, dp, dl, pout, opitch, ol, prm, st)
        if prm is None:
            return self.lib.meao_execute_batch(ctx, n_real, pin, dl, pout, ol, st)
        return self.lib.meao_execute_batch_params(ctx, n_real, pin, dl, pout, ol, prm, st)

    def call_prefetch(self, op, bad=None):
        de = np.dtype(self.depth_dt).itemsize
        w = op.size[0] if op.size else self.w                         # the pitch of a sized announcement: texels of ITS width
        dp = (M.row_texels(op.pitch, w)) * de if op.pitch else 0
        din = [self.depth_surface(b).ptr() for b in op.bufs]
        n = len(din)
        prm = None if op.params is None else self.params_ctypes(op.params)
        if bad == "sized_bad_pitch":
            dp = w * de - de                                          # below the announced row
        if op.size:
            pin = (C.c_void_p * n)(*din)
            if self.G:
                return self.lib.meao_pool_prefetch_batch_sized(self.ao._pool, op.size[0], op.size[1], n, pin, dp, prm)
            return self.lib.meao_prefetch_batch_sized(self.ao._ctx, op.size[0], op.size[1], n, pin, dp, prm)
        if bad == "bad_pitch":
            dp = self.w * de - de
        if bad == "null_pointer":
            din[0] = None
        if bad == "n_zero":
            n = 0
        if bad == "n_over":
            n = self.P.max_batch * (self.G or 1) + 1
            din = (din * n)[:n]
        pin = (C.c_void_p * max(1, len(din)))(*din)
        if self.G:
            p = self.ao._pool
            if dp:
                return self.lib.meao_pool_prefetch_batch_pitched(p, n, pin, dp, prm)
            return self.lib.meao_pool_prefetch_batch(p, n, pin) if prm is None else self.lib.meao_pool_prefetch_batch_params(p, n, pin, prm)
        ctx = self.ao._ctx
        if dp:
            return self.lib.meao_prefetch_batch_pitched(ctx, n, pin, dp, prm)
        return self.lib.meao_prefetch_batch(ctx, n, pin) if prm is None else self.lib.meao_prefetch_batch_params(ctx, n, pin, prm)

    def frame_inputs(self, op):
        """[(oracle frame, fields)] of an execute, from the bytes the call is given under the pitch it is given."""
        out = []
        for f, (b, (w, h, pitch, _)) in enumerate(zip(op.bufs, self.geometry(op))):
            s = self.depth[b]
            frame = Surface.view(s.oracle_bytes, np.float32 if self.linear else self.depth_dt, pitch, w, h)
            fields = self.ctx_fields if op.params is None else self.fields_for(op.params[f])
            out.append((frame, fields))
        return out

    def set_profiling(self):
        for c in self.members:
            L.check(self.lib.meao_set_profiling(c, 1), c)

    def pass_times(self, c):
        ms, cnt = (C.c_float * L.NUM_PASSES)(), C.c_int32()
        L.check(self.lib.meao_get_pass_times(c, C.byref(ms), C.byref(cnt)), c)
        return list(ms), cnt.value

    def note_fusable(self, op, expects):
        """Counts the carried passes that MAY run inside their carrier's last kernel, by what include/meao.h says of it: never
        what a mixed call carries, else M.header_lets_it_ride (every surface here is aligned).  An upper bound on the fused launches of a trace, not their number: whether an eligible pass does ride is decided
        by host code the header leaves free ("host code decides, no kernel knows" -- the tile height of the last kernel)."""
        G = self.G or 1
        for m, e in enumerate(expects):
            if e is None or e.carried is None or "mixed_call" in e.events or self.own_launch:
                continue
            self.fusable += M.header_lets_it_ride(e.carried, len(op.bufs[m::G]), (self.w, self.h),
                                                  self.fmt in (L.DEPTH_F32, L.DEPTH_LINEAR_F32))

    def execute(self, op, expect):
        expects = self.member_expects(expect)
        self.note_fusable(op, expects)
        self.switch_stream(op.stream)
        if self.stepped:
            self.set_profiling()
        inputs = self.frame_inputs(op)
        status = self.call_execute(op)
        assert status == L.OK, (op, status, self.lib.meao_last_error(self.members[0]))
        geo = self.geometry(op)
        host_want = []
        for f, (frame, fields) in enumerate(inputs):
            w, h, _, opitch = geo[f]
            want = self.want(frame, fields)["result"]
            if op.out_host:                                           # the device surface of that id is not touched
                host_want.append(self.outs[op.outs[f]].mirror.copy())
                Surface.view(host_want[-1], self.ao_dt, opitch, w, h)[:] = want
            else:
                Surface.view(self.outs[op.outs[f]].mirror, self.ao_dt, opitch, w, h)[:] = want
        if not self.stepped:
            self.checks += [("out", o, g[3], g[0], g[1], op) for o, g in zip(op.outs, geo)]
            self.check_composites(op, expects)
            return
        self.sync()
        for f, o in enumerate(op.outs):
            view = (geo[f][3], geo[f][0], geo[f][1])
            if op.out_host:
                self.compare_bytes(self.host_out[f], host_want[f], op, f, "HOST result", view)
            else:
                self.compare_surface(self.outs[o], op, f, "result", view)
        if not op.depth_host:
            for f, b in enumerate(op.bufs):                         # depth surfaces are read, never written
                self.compare_surface(self.depth[b], op, f, "depth surface", None)
        # pass times: what the header gives (see the module docstring of tests/call_model.py)
        for m, e in enumerate(expects):
            ms, cnt = self.pass_times(self.members[m])
            if e is None:
                assert cnt == 0, (op, m, "a member that is dealt no frame launches nothing", cnt)
                continue
            assert cnt == 1, (op, m, cnt)
            if e.own_pass:
                assert ms[PASS_DOWNSAMPLE] > 0, (op, m, "the call's own downsample pass must run", e.refused, ms)
            elif e.carried is None:
                assert ms[PASS_DOWNSAMPLE] == 0, (op, m, "a reused pass and nothing announced: no downsample launch", ms)
            elif self.own_launch:
                assert ms[PASS_DOWNSAMPLE] > 0, (op, m, "the carried pass as a launch of its own", ms)
            if "mixed_call" in e.events:                             # its own pass, and what it carries behind it, in both modes
                assert e.own_pass and e.per_frame and ms[PASS_DOWNSAMPLE] > 0, (op, m, "a mixed call runs its own downsample pass", ms)
        self.check_composites(op, expects)
        self.check_hostile(op, expects)
        if op.read_debug:
            self.check_debug(op, inputs)
        self.last_read = (op, [(frame.copy(), fields) for frame, fields in inputs], expects)

    def compare_bytes(self, got, want, op, f, what, view):
        """Every byte of a surface.  view: (row stride, width, height) of the frame in it, in texels, for the report alone."""
        if not np.array_equal(got, want):
            frame_g = Surface.view(got, self.ao_dt, *view) if view else got
            frame_w = Surface.view(want, self.ao_dt, *view) if view else want
            inside = not np.array_equal(frame_g, frame_w)
            raise AssertionError((op, "frame %d" % f, what, "texels differ" if inside else "bytes OUTSIDE the frame changed",
                                  int((got != want).sum()), self.log[-6:]))

    def compare_surface(self, s, op, f, what, view):
        self.compare_bytes(s.dev.cpu().numpy(), s.mirror, op, f, what, view)

    def check_hostile(self, op, expects):
        """Known by construction only: inside the exact range, a frame with hostile level texels has its bit, a clean one has not."""
        if self.fmt == L.DEPTH_UNORM16:
            return
        geo = self.geometry(op)
        G = self.G or 1
        for m, e in enumerate(expects):
            if e is None or not e.exact:
                continue
            mask = C.c_uint64()
            L.check(self.lib.meao_hostile_frames(self.members[m], C.byref(mask)), self.members[m])
            for i, b in enumerate(op.bufs[m::G]):                   # one bit per frame of the member's share, in frame order
                content, laid = self.laid.get(b, (("unknown", 0), None))
                w, h, rows, _ = geo[m + i * G]
                if laid != (rows, w, h):
                    continue                                        # read under another pitch than it was written: not a known frame
                bit = mask.value >> i & 1
                if content[0] == "hostile_level":
                    assert bit == 1, (op, m, i, "hostile level texels: bit must be set", hex(mask.value), e.reused)
                elif content[0] == "synth":
                    assert bit == 0, (op, m, i, "clean frame: bit must be clear", hex(mask.value), e.reused)

    def debug_buffer(self, f, debug_id, size=None):
        """meao_get_intermediate of frame f of the last call: slot f // G of member f mod G.  size: the frame's own, after a mixed
        call -- the buffer is then described by the call that returns it, and room is made for the largest the member can hold."""
        G = self.G or 1
        ctx, slot = self.members[f % G], f // G
        d = L.Desc()
        if size is not None:
            cfg, cw, ch = L.Config(), C.c_int32(), C.c_int32()
            L.check(self.lib.meao_get_config(ctx, C.byref(cfg)), ctx)
            L.check(self.lib.meao_get_capacity(ctx, C.byref(cw), C.byref(ch)), ctx)
            cfg.width, cfg.height = max(cw.value, cfg.width), max(ch.value, cfg.height)
            L.check(self.lib.meao_describe_buffer(C.byref(cfg), debug_id, C.byref(d)))
            raw = np.empty(d.bytes, np.uint8)
            L.check(self.lib.meao_get_intermediate(ctx, slot, debug_id, raw.ctypes.data, raw.nbytes, L.MEM_HOST, C.byref(d)), ctx)
            dt = {L.FMT_F32: np.float32, L.FMT_F16: np.uint16, L.FMT_UNORM8: np.uint8}[d.format]
            return raw[:d.bytes].view(dt).reshape((d.slices, d.height, d.width) if d.slices > 1 else (d.height, d.width))
        L.check(self.lib.meao_get_intermediate(ctx, slot, debug_id, None, 0, L.MEM_HOST, C.byref(d)), ctx)
        out = np.empty((d.slices, d.height, d.width) if d.slices > 1 else (d.height, d.width),
                       {L.FMT_F32: np.float32, L.FMT_F16: np.uint16, L.FMT_UNORM8: np.uint8}[d.format])
        L.check(self.lib.meao_get_intermediate(ctx, slot, debug_id, out.ctypes.data, out.nbytes, L.MEM_HOST, C.byref(d)), ctx)
        return out

    def check_debug(self, op, inputs, why="", view=False):
        """One frame of the last execute, three debug ids (one of 1-9 always), against the oracle under the parameters THAT CALL
        used for the frame -- whatever the context's are by now."""
        n = len(op.bufs)
        f = self.rng.randrange(n)
        ids = H.valid_debug_ids(4, self.hq)
        pick = [self.rng.choice(range(1, 10))] + self.rng.sample(ids, 2)
        frame, fields = inputs[f]
        want = self.want(frame, fields, full=True)
        mixed = self.is_mixed(op)
        for i in pick:
            got = self.debug_buffer(f, i, frame.shape[::-1] if mixed else None)
            # (after a mixed call: frame f's buffers at frame f's size -- the oracle's at that size)
            assert got.shape == want[H.NAMES[i]].shape, (op, why, "debug id %d of frame %d" % (i, f), got.shape, want[H.NAMES[i]].shape)
            ok, _ = H.nan_aware_equal(got, want[H.NAMES[i]])
            assert ok, (op, why, "debug id %d of frame %d" % (i, f), H.diff_report(H.NAMES[i], got, want[H.NAMES[i]]), self.log[-6:])
        if self.G:
            return
        if n < self.P.max_batch:                                     # a slot the last execute did not produce
            with pytest.raises(L.MeaoError) as err:
                self.ao.debug_buffer(2, frame=n)
            assert err.value.status == L.ERR_INVALID_ARGUMENT
        if view or not self.viewed:
            self.viewed = True
            i = pick[0]
            got = np.empty(frame.shape, self.ao_dt)                 # meao_debug_view: the frame's own size after a mixed call
            L.check(self.lib.meao_debug_view(self.ao._ctx, f, i, got.ctypes.data, L.MEM_HOST, None), self.ao._ctx)
            wantv = self.O.debug_view(want, i, self.settings(fields, frame.shape[1], frame.shape[0]))
            ok, _ = H.nan_aware_equal(got, wantv)
            assert ok, (op, why, "debug view %d of frame %d" % (i, f), H.diff_report("view", got, wantv))

    def reread(self, why):
        """'As left by the last execute' some operations later (meao_set_params, meao_debug_set, an invalid call in between): the
        debug buffers, a debug view and the hostile mask of that call, under ITS parameters."""
        if not self.stepped or self.last_read is None:
            return
        op, inputs, expects = self.last_read
        models = self.model.members if self.G else [self.model]
        G = self.G or 1
        for m, c in enumerate(models[:len(op.bufs)]):
            if not c.readable() or c.last.bufs != tuple(op.bufs[m::G]):
                return
        self.check_hostile(op, expects)
        self.check_debug(op, inputs, why=why, view=True)

    def assert_refuses_debug(self, op):
        """'As left by the last execute' is gone: every member refuses meao_get_intermediate."""
        for c in self.members:
            d = L.Desc()
            L.check(self.lib.meao_get_intermediate(c, 0, 2, None, 0, L.MEM_HOST, C.byref(d)), c)      # the description alone
            out = np.empty(d.bytes, np.uint8)
            status = self.lib.meao_get_intermediate(c, 0, 2, out.ctypes.data, out.nbytes, L.MEM_HOST, C.byref(d))
            assert status == L.ERR_INVALID_ARGUMENT, (op, status)

    def check_geometry(self, op):
        """Every member has the model's size and the model's reservation (meao_get_config, meao_get_capacity)."""
        models = self.model.members if self.G else [self.model]
        for m, c in enumerate(self.members):
            cfg, cw, ch = L.Config(), C.c_int32(), C.c_int32()
            L.check(self.lib.meao_get_config(c, C.byref(cfg)), c)
            L.check(self.lib.meao_get_capacity(c, C.byref(cw), C.byref(ch)), c)
            assert (cfg.width, cfg.height) == (models[m].width, models[m].height), (op, m, "size", cfg.width, cfg.height)
            assert (cw.value, ch.value) == models[m].cap, (op, m, "capacity", cw.value, ch.value, models[m].cap)

    def comp_enqueue(self, op, expect):
        expects = self.member_expects(expect)
        n = len(op.bufs)
        ao_ptrs, col_ptrs = [], []
        for o, c in zip(op.bufs, op.colors):
            s = self.surface(self.colors, c, self.cap * 8, 0)
            base = self.color0(c)
            s.mirror[:base.nbytes] = base.reshape(-1).view(np.uint8)
            if self.stepped or self.G:
                s.dev.copy_(self.torch.from_numpy(s.mirror))
            else:
                with self.on_stream():
                    s.dev.copy_(self.library[("color", c, (self.w, self.h))], non_blocking=True)   # put there by prepare()
            ao = Surface.view(self.outs[o].mirror, self.ao_dt, self.w, self.w, self.h).copy()
            want = base.copy()
            self.O.composite(ao, want, op.mode, self.ao_fmt)
            self.color_want[c] = want
            self.final_color.pop(c, None)
            ao_ptrs.append(self.outs[o].ptr())
            col_ptrs.append(s.ptr())
        self.ao.composite_enqueue_device(op.mode, ao_ptrs, col_ptrs)
        self.check_composites(op, expects)

    def invalid(self, op, expect):
        expects = self.member_expects(expect)
        before = self.pending()
        if op.on == "reserve":
            status = (self.lib.meao_pool_reserve(self.ao._pool, *op.size) if self.G else self.lib.meao_reserve(self.ao._ctx, *op.size))
        elif op.on == "resize":
            status = (self.lib.meao_pool_resize(self.ao._pool, *op.size) if self.G else self.lib.meao_resize(self.ao._ctx, *op.size))
        else:
            status = self.call_execute(op, bad=op.what) if op.on == "execute" else self.call_prefetch(op, bad=op.what)
        assert status == expects[0].status, (op, status)
        assert self.pending() == before, (op, "an invalid call must leave a waiting composite waiting")
        if op.what in M.SIZED_INVALID:
            self.check_geometry(op)

    def run(self, ops, model):
        self.model = model
        if M.initial_cap(self.P) != (0, 0):                          # a free-running sequence starts reserved
            self.ao.reserve(*self.P.reserve)
            self.check_geometry("the reservation before the first operation")
        self.prepare(ops)
        for op in ops:
            expect = model.apply(op)
            self.log.append((op.kind, op.bufs, op.pitch, op.stream))
            k = op.kind
            if k == "refill":
                self.refill(op)
            elif k == "execute":
                self.execute(op, expect)
            elif k == "prefetch":
                assert self.call_prefetch(op) == L.OK, op
                if self.stepped and not self.G and self.member_expects(expect)[0].reallocated:
                    self.assert_refuses_debug(op)
                    self.check_geometry(op)                          # the reservation survives the re-allocation
            elif k == "set_params":
                self.apply_params(self.fields_for(op.param))
                self.reread("after set_params")
            elif k == "resize":
                self.ao.resize(*op.size)
                self.check_composites(op, self.member_expects(expect))      # it ran at the old size
                self.w, self.h = op.size
                self.last_read = None
                self.check_geometry(op)
                if self.stepped:
                    self.assert_refuses_debug(op)
            elif k == "reserve":
                self.ao.reserve(*op.size)
                self.last_read = None
                self.check_geometry(op)
                self.assert_refuses_debug(op)
                self.check_composites(op, self.member_expects(expect))      # none ran: a waiting batch stays waiting
            elif k == "comp_enqueue":
                self.comp_enqueue(op, expect)
            elif k == "comp_flush":
                self.ao.composite_flush()
                self.check_composites(op, self.member_expects(expect))
            elif k == "debug_set":
                self.ao.debug_set(op.key, op.value)
                self.reread("after debug_set")
            elif k == "invalid":
                self.invalid(op, expect)
                self.reread("after an invalid call")
        self.sync()
        self.finish()

    def finish(self):
        """Free-running: everything the sequence wrote, compared once it has all run."""
        seen = set()
        for chk in self.checks:
            if chk[0] == "out":
                _, o, pitch, w, h, op = chk
                if o not in seen:
                    seen.add(o)
                    self.compare_surface(self.outs[o], op, 0, "result (buffer %d)" % o, (pitch, w, h))
        for c, want in self.final_color.items():
            got = self.colors[c].dev.cpu().numpy()[:want.nbytes].view(np.uint16).reshape(want.shape)
            assert np.array_equal(got, want), ("composite of colour %d" % c, H.diff_report("color", got, want))
        assert not self.color_want or self.pending() > 0, "the model has a composite waiting at the end, the library has none"

    def totals(self):
        models = self.model.members if self.G else [self.model]
        return dict({k: sum(m.totals[k] for m in models) for k in models[0].totals}, fusable=self.fusable)

    def close(self):
        self.ao.close(flush_composite=True)


@pytest.fixture(scope="module")
def lin_c():
    from tests.linear_depth import linearize
    return linearize()


# ---- stepped sequences on one context

@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.CASES))
def test_stepped_sequence(oracle, lin_c, name, own_launch):
    ops, model = M.case_sequence("stepped", name)
    d = Driver(oracle, M.CASES[name], M.STEPPED, own_launch, lin_c, stepped=True, seed=M.CASES[name]["seed"])
    try:
        d.run(ops, model)
    finally:
        d.close()


# ---- the pool, stepped

@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.POOL_CASES))
def test_pool_stepped_sequence(oracle, name, own_launch):
    ops, model = M.case_sequence("pool_stepped", name)
    c = M.POOL_CASES[name]
    d = Driver(oracle, c, M.Profile(pool=c["members"], **M.POOL), own_launch, stepped=True)
    try:
        d.run(ops, model)
    finally:
        d.close()


def test_pool_member_that_sat_a_call_out_holds_no_announcement(oracle):
    """Three members; B (three frames) is announced, A (two frames) executed, then B.  Member 2 sat A out.  It must not be left
    with B's announcement: carried by the very call that processes B, it would leave a ready set keyed on B's buffer, and the
    next call on the refilled buffer would build member 2's frame from the old depth levels."""
    import torch
    from miniengineao_amd import AmbientOcclusionPool
    w, h = 384, 256
    s = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    A = [synth.make("S2", w, h, seed=500 + f) for f in range(2)]
    B0 = [synth.make("S2", w, h, seed=510 + f) for f in range(3)]
    B1 = [synth.make("S2", w, h, seed=520 + f) for f in range(3)]
    a = [torch.from_numpy(x).to(dev) for x in A]
    b = [torch.from_numpy(x).to(dev) for x in B0]
    outs = [[torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(3)] for _ in range(3)]
    lib = L.load()
    with AmbientOcclusionPool(w, h, [0, 0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                              reversed_z=s.reversed_z, pipelined=True) as pool:
        pb = [t.data_ptr() for t in b]
        pool.prefetch_device(pb)
        pool.execute_device([t.data_ptr() for t in a], [t.data_ptr() for t in outs[0][:2]])
        pool.execute_device(pb, [t.data_ptr() for t in outs[1]])
        pool.synchronize()
        for t, x in zip(b, B1):                                        # B's buffers are the host's again: new frames, same pointers
            t.copy_(torch.from_numpy(x))
        torch.cuda.synchronize(dev)
        for m in range(3):
            L.check(lib.meao_set_profiling(pool.member_context(m), 1))
        pool.execute_device(pb, [t.data_ptr() for t in outs[2]])
        pool.synchronize()
        for m in range(3):
            ms, cnt = (C.c_float * L.NUM_PASSES)(), C.c_int32()
            L.check(lib.meao_get_pass_times(pool.member_context(m), C.byref(ms), C.byref(cnt)))
            assert cnt.value == 1 and ms[PASS_DOWNSAMPLE] > 0, (m, list(ms))     # nothing was announced for this call
    for k, frames in ((0, A), (1, B0), (2, B1)):
        for f, x in enumerate(frames):
            want = oracle.run(x, s, result_only=True)["result"]
            got = outs[k][f].cpu().numpy()
            assert np.array_equal(got, want), (k, f, H.diff_report("result", got, want))


# ---- hand-written histories that must not depend on a seed

@pytest.mark.parametrize("how", ["set_params", "resize"])
def test_announcement_does_not_survive_set_params_or_resize(oracle, how):
    """Announce B, then meao_set_params / meao_resize, execute A, execute B: A carries nothing, so B finds nothing ready and runs
    its own pass (the DOWNSAMPLE slot is > 0 in both calls) with the parameters and the geometry of ITS call."""
    import torch
    w0, h0 = 384, 256
    w, h = (380, 250) if how == "resize" else (w0, h0)
    dev = torch.device("cuda", 0)
    before, after = fields_of(0, w0, h0), fields_of(2 if how == "set_params" else 0, w, h)      # tag 2: another near / far
    if how == "resize":
        after["proj00"] = before["proj00"]                         # meao_resize keeps the context's parameters
    s_after = oracle.Settings(w, h, **after)
    A = [synth.make("S2", w, h, seed=700 + f) for f in range(2)]
    B = [synth.make("S2", w, h, seed=710 + f) for f in range(2)]
    cap = w0 * h0
    def surf(x):
        t = torch.zeros(cap, dtype=torch.float32, device=dev)
        t[:x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
        return t
    a, b = [surf(x) for x in A], [surf(x) for x in B]
    outs = [[torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(2)] for _ in range(2)]
    ao = H.component(oracle.Settings(w0, h0, **before), max_batch=2, pipelined=True, debug={L.DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH: 1})
    try:
        ao._sync_params()
        ao.prefetch_device([t.data_ptr() for t in b])
        if how == "set_params":
            p = to_params(frame_params_of(after), ao._prm)
            L.check(ao._lib.meao_set_params(ao._ctx, C.byref(p)), ao._ctx)
        else:
            ao.resize(w, h)
        ms_a = downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in a], [t.data_ptr() for t in outs[0]]))
        ms_b = downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in b], [t.data_ptr() for t in outs[1]]))
        assert ms_a > 0 and ms_b > 0, (ms_a, ms_b)
        ms_c = downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in b], [t.data_ptr() for t in outs[1]]))
        assert ms_c > 0, ms_c                                        # and nothing was left ready by B either
        ao.synchronize()
        for k, frames in enumerate((A, B)):
            for f, x in enumerate(frames):
                want = oracle.run(x, s_after, result_only=True)["result"]
                got = outs[k][f].cpu().numpy()[:w * h].reshape(h, w)
                assert np.array_equal(got, want), (k, f, H.diff_report("result", got, want))
    finally:
        ao.close()


def test_linear_depth_reuse_key_is_the_far_plane_alone(oracle, lin_c):
    """MEAO_DEPTH_LINEAR_F32: 'a prefetched downsample pass is reused when each frame's s matches', s = the f32 nearest 1 / far_clip.
    A frame announced with far 128 and asked for with far 64 (and linearised by THAT camera) is refused; announced with far 128
    and asked for with another near plane and Z direction but far 128 is reused.  Both equal the oracle of the asking camera."""
    import torch
    from tests.linear_depth import to_linear
    w, h = 384, 256
    dev = torch.device("cuda", 0)
    ann = fields_of(0, w, h)                                          # near 0.1, far 128, reversed Z
    cases = {"other_far": (fields_of(2, w, h), False),                # near 0.1, far 64
             "same_far_other_near_and_direction": (fields_of(3, w, h), True)}     # near 0.1 -> conventional Z, far 128
    cases["same_far_other_near_and_direction"][0]["near_clip"] = 0.25
    raw = synth.make("S2", w, h, seed=730)
    other = torch.from_numpy(to_linear(lin_c, synth.make("S2", w, h, seed=731), CAM_LINEAR)[1]).to(dev)
    for name, (ask, reused) in cases.items():
        cam = synth.Camera(near=ask["near_clip"], far=ask["far_clip"], reversed_z=ask["reversed_z"])
        d, z = to_linear(lin_c, raw, cam)
        zt = torch.from_numpy(z).to(dev)
        out = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(2)]
        ao = H.component(oracle.Settings(w, h, **ann), max_batch=1, pipelined=True, depth_format=L.DEPTH_LINEAR_F32)
        try:
            ao._sync_params()
            ao.prefetch_device([zt.data_ptr()], params=[frame_params_of(ann)])
            ao.execute_device([other.data_ptr()], [out[0].data_ptr()])
            ms = downsample_ms(ao, lambda: ao.execute_device([zt.data_ptr()], [out[1].data_ptr()], params=[frame_params_of(ask)]))
            assert (ms == 0) == reused, (name, ms)
            ao.synchronize()
            want = oracle.run(d, oracle.Settings(w, h, **ask), result_only=True)["result"]
            got = out[1].cpu().numpy()
            assert np.array_equal(got, want), (name, H.diff_report("result", got, want))
        finally:
            ao.close()


# ---- the ring of eight per-frame constant tables

def test_ring_of_frame_tables_wraps_with_the_host_ahead(oracle):
    """24 consecutive per-frame calls on one stream, every frame of every call with parameters of its own, every other call also
    carrying a per-frame announcement, n varying, behind a delay on the stream so that the host is more than eight calls ahead of
    the device: the ninth call must wait for the first (the documented back-pressure), and no call may render with another
    call's table.  The precondition -- the first call has not completed when the eighth has returned -- is asserted.
    The delay is twenty times the time the host needs to submit eight calls (measured in the same run), at least 40 ms and at
    most 400 ms.  Measured on an MI355X: eight calls are submitted in 0.32 - 0.35 ms, so the 40 ms floor applies (more than a
    hundred times the submit time); the eighth call had returned 0.31 - 0.37 ms after the first was submitted, and the ninth
    returned after 32.5 - 33.6 ms, when the delay had run out and the first call had completed."""
    import torch
    w, h, mb, calls = 384, 256, 4, 24
    base = H.settings(oracle, w, h)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ns = [1 + (5 * i + i // 3) % mb for i in range(calls)]
    tags = [0, 1, 2, 3, 4, 5]

    def fields(i, f):
        fl = fields_of(tags[(i + f) % len(tags)], w, h)
        fl["intensity"] = float(np.float32(0.25 + 0.01 * (4 * i + f)))           # no two frames of the test share a table
        return fl
    frames = [[synth.make("S2", w, h, seed=600 + (4 * i + f) % 7) for f in range(ns[i])] for i in range(calls)]
    dd = [[torch.from_numpy(x).to(dev) for x in fr] for fr in frames]
    out = [[torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(ns[i])] for i in range(calls)]
    prm = [[frame_params_of(fields(i, f)) for f in range(ns[i])] for i in range(calls)]
    ao = H.component(base, max_batch=mb, pipelined=True)
    try:
        ao._sync_params()
        st = stream.cuda_stream

        def submit(i, outs):
            if i % 2 == 0 and i + 1 < calls:
                ao.prefetch_device([t.data_ptr() for t in dd[i + 1]], params=prm[i + 1])
            ao.execute_device([t.data_ptr() for t in dd[i]], [t.data_ptr() for t in outs], st, params=prm[i])
        # the time the host needs to submit eight calls (also warms everything up; the ring is empty again afterwards)
        scratch = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(mb)]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(8):
            ao.execute_device([t.data_ptr() for t in dd[i]], [t.data_ptr() for t in scratch[:ns[i]]], st, params=prm[i])
        submit_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
        # cycles of torch.cuda._sleep per millisecond on this device
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            torch.cuda._sleep(20_000_000)
            e1.record()
        torch.cuda.synchronize(dev)
        per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
        delay_ms = min(400.0, max(40.0, 20.0 * submit_ms))
        first = torch.cuda.Event()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(delay_ms * per_ms))
        t0 = time.perf_counter()
        for i in range(calls):
            submit(i, out[i])
            if i == 0:
                first.record(stream)
            if i == 7:
                ahead_ms = (time.perf_counter() - t0) * 1e3
                assert not first.query(), ("the host is not eight calls ahead of the device: the test proves nothing",
                                           submit_ms, delay_ms, ahead_ms)
            if i == 8:
                blocked_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
        print("ring wrap: submit of eight calls %.2f ms, delay %.1f ms, eight calls ahead after %.2f ms, ninth returned after %.1f ms"
              % (submit_ms, delay_ms, ahead_ms, blocked_ms))
        assert blocked_ms >= 0.5 * delay_ms, ("the ninth call did not wait for the first", blocked_ms, delay_ms)
        for i in range(calls):
            for f in range(ns[i]):
                s = dataclasses.replace(base, **fields(i, f))
                want = oracle.run(frames[i][f], s, result_only=True)["result"]
                got = out[i][f].cpu().numpy()
                assert np.array_equal(got, want), ("call %d frame %d" % (i, f), H.diff_report("result", got, want))
    finally:
        ao.close()


# ---- free-running sequences: launches by kernel name

CHILD = r"""
import json
import sys
from oracle import oracle as O
from tests import call_model as M
from tests import test_call_sequences_gpu as T          # the child's own parent module: the driver stays in its suite

kind, name, own_launch = sys.argv[1], sys.argv[2], int(sys.argv[3])
O.build()
ops, model = M.case_sequence(kind, name)
lin_c = None
cfg, prof, _ = M.case_profile(kind, name)
if cfg.get("linear"):
    from tests.linear_depth import linearize
    lin_c = linearize()
d = T.Driver(O, cfg, prof, own_launch, lin_c, stepped=False)
try:
    d.run(ops, model)
    print("MODEL " + json.dumps(d.totals()))
finally:
    d.close()
"""


def trace_counts(k):
    standalone = sum(1 for n in k.short if re.match(r"downsample\w*_kernel", n))
    fused = sum(1 for n in k.short if n.startswith("upsample_final_with_next_downsample"))
    rwc = sum(1 for n in k.short if n.startswith("render_with_composite_kernel"))
    plain = sum(1 for n in k.short if n.startswith("composite_kernel"))
    return standalone, fused, rwc, plain


def run_free(tmp_path, kind, name, own_launch):
    k = H.kernel_trace(tmp_path, CHILD, args=(kind, name, str(own_launch)))
    line = [ln for ln in k.stdout.splitlines() if ln.startswith("MODEL ")]
    assert line, k.stdout[-2000:] + k.stderr[-2000:]
    model = json.loads(line[-1][6:])
    standalone, fused, rwc, plain = trace_counts(k)
    assert standalone + fused == model["own"] + model["carried"], (standalone, fused, model)
    assert rwc == model["comp_carried_launches"] and plain == model["comp_plain_launches"], (rwc, plain, model)
    if own_launch:
        assert fused == 0, (fused, model)
    return standalone, fused, model


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.FREE_CASES))
def test_free_running_sequence(tmp_path, name, own_launch):
    standalone, fused, model = run_free(tmp_path, "free", name, own_launch)
    if not own_launch and M.FREE_CASES[name].get("depth", "f32") in ("f32", "linear_f32"):
        assert fused > 0, (fused, model)            # width % 8 == 0, f32 texels: the fused form exists and is used
        # an announcement with more frames than its carrier cannot ride: it is among the stand-alone launches
        assert model["carried_more"] > 0 and standalone >= model["own"] + model["carried_more"], (standalone, fused, model)


@pytest.mark.parametrize("name", sorted(M.POOL_CASES))
def test_pool_free_running_sequence(tmp_path, name):
    run_free(tmp_path, "pool_free", name, 0)
