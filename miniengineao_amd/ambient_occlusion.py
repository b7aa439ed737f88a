"""Host-side mirror of the reference component ``MiniEngineAO.AmbientOcclusion``
(Assets/MiniEngineAO/AmbientOcclusion.cs, "AO.cs") over the C ABI of libmeao_hip.so.

The reference is a Unity MonoBehaviour: six public properties (AO.cs:22-66), implicit camera
inputs (AO.cs:339-340,563-573), depth texture in, "AmbientOcclusion" R8 texture out
(AO.cs:475,824).  This class keeps the property names and meaning; what Unity did implicitly
(camera, depth texture, render-texture output) is explicit here.  Property changes are picked
up lazily before the next frame, like CheckPropertiesChanged (AO.cs:104-113).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib as L
from .frame_params import FrameParams, params_array

_NP_OF_FMT = {L.FMT_F32: np.float32, L.FMT_F16: np.uint16, L.FMT_UNORM8: np.uint8}
# element type of the depth frames per meao_depth_format: numpy host arrays, torch tensors (by name: torch is imported lazily)
DEPTH_NUMPY = {L.DEPTH_F32: np.float32, L.DEPTH_UNORM16: np.uint16, L.DEPTH_UNORM24: np.uint32, L.DEPTH_F16: np.uint16,
               L.DEPTH_LINEAR_F32: np.float32, L.DEPTH_LINEAR_F16: np.float16}
DEPTH_TORCH = {L.DEPTH_F32: "float32", L.DEPTH_UNORM16: "uint16", L.DEPTH_UNORM24: "int32", L.DEPTH_F16: "float16",
               L.DEPTH_LINEAR_F32: "float32", L.DEPTH_LINEAR_F16: "float16"}

# _debug values (AO.cs:789-808)
DEBUG_BUFFER_NAMES = {
    1: "LinearDepth", 2: "LowDepth1", 3: "LowDepth2", 4: "LowDepth3", 5: "LowDepth4",
    6: "TiledDepth1", 7: "TiledDepth2", 8: "TiledDepth3", 9: "TiledDepth4",
    10: "Occlusion1", 11: "Occlusion2", 12: "Occlusion3", 13: "Occlusion4",
    14: "Combined1", 15: "Combined2", 16: "Combined3", 17: "AmbientOcclusion",
}
# beyond the reference's list: the Render.main (wide) targets of the hq_levels variant
HQ_BUFFER_NAMES = {18: "OcclusionHQ1", 19: "OcclusionHQ2", 20: "OcclusionHQ3", 21: "OcclusionHQ4"}


def extents_array(extents: Sequence[tuple], n: int):
    """[(width, height[, depth_pitch, ao_pitch]), ...] -> the meao_extent array of meao_execute_batch_extents (pitches in bytes,
    0 or absent = packed for that frame's width)."""
    if len(extents) != n:
        raise ValueError(f"{len(extents)} extents for {n} frames")
    arr = (L.Extent * n)()
    for f, e in enumerate(extents):
        if len(e) not in (2, 4):
            raise ValueError(f"extents[{f}]: expected (width, height) or (width, height, depth_pitch, ao_pitch)")
        arr[f].width, arr[f].height = int(e[0]), int(e[1])
        arr[f].depth_pitch, arr[f].ao_pitch = (int(e[2]), int(e[3])) if len(e) == 4 else (0, 0)
    return arr


def target_extents_array(extents: Sequence[tuple], n: int):
    """[(width, height[, ao_pitch, color_pitch, gbuffer0_pitch]), ...] -> the meao_target_extent array of
    meao_composite_batch_extents (pitches in bytes, 0 or absent = packed for that frame's width)."""
    if len(extents) != n:
        raise ValueError(f"{len(extents)} extents for {n} frames")
    arr = (L.TargetExtent * n)()
    for f, e in enumerate(extents):
        if len(e) not in (2, 5):
            raise ValueError(f"extents[{f}]: expected (width, height) or (width, height, ao_pitch, color_pitch, gbuffer0_pitch)")
        arr[f].width, arr[f].height = int(e[0]), int(e[1])
        arr[f].ao_pitch, arr[f].color_pitch, arr[f].gbuffer0_pitch = (int(e[2]), int(e[3]), int(e[4])) if len(e) == 5 else (0, 0, 0)
    return arr


def _pitch_array(pitches: Optional[Sequence[int]], n: int, what: str):
    """One row pitch in bytes per frame -> the uint64 array of meao_execute_batch_extents_shaded; None = every frame packed."""
    if pitches is None:
        return None
    if len(pitches) != n:
        raise ValueError(f"{len(pitches)} {what} for {n} frames")
    return (C.c_uint64 * n)(*[int(v) for v in pitches])


class AmbientOcclusion:
    """depth in -> AO texture out, on one MI355X.  One instance per device."""

    def __init__(self, width: int, height: int, *, device: int = 0, num_levels: int = 4,
                 ao_format: int = L.AO_R8, f16_rounding: int = L.F16_RTZ_CLAMP,
                 max_batch: int = 1, depth_format: int = L.DEPTH_F32,
                 near_clip: float = 0.3, far_clip: float = 1000.0,
                 projection00: Optional[float] = None, reversed_z: bool = True,
                 hq_levels: int = 0, sample_set: int = L.SAMPLES_CHECKER, single_pass_stereo: bool = False,
                 pipelined: bool = False):
        """hq_levels / sample_set / single_pass_stereo: variants the reference's shaders and host carry
        but its command buffer never (or only in VR) uses; see include/meao.h.  ``width`` is the
        double-wide eye pair when single_pass_stereo is set (AO.cs:339)."""
        self._lib = L.load()
        cfg = L.Config()
        self._lib.meao_default_config(C.byref(cfg))
        cfg.device, cfg.width, cfg.height = device, width, height
        cfg.num_levels, cfg.ao_format, cfg.f16_rounding = num_levels, ao_format, f16_rounding
        cfg.max_batch = max_batch
        cfg.depth_format = depth_format
        cfg.hq_levels, cfg.sample_set = hq_levels, sample_set
        cfg.pipelined = 1 if pipelined else 0   # second downsample set from the start (prefetch_device never allocates)
        self._cfg = cfg
        prm = L.Params()
        self._lib.meao_default_params(C.byref(prm))
        prm.near_clip, prm.far_clip = near_clip, far_clip
        if projection00 is not None:
            prm.proj00 = projection00
        prm.reversed_z = 1 if reversed_z else 0
        prm.single_pass_stereo = 1 if single_pass_stereo else 0
        self._prm = prm
        self._ambient_only = True          # AO.cs:68; composite-only flag, kept for surface parity
        self._debug = 0                    # AO.cs:60
        self._dirty = True
        self._last_sizes = None            # [(width, height)] of the frames of the last call where it was a mixed-size batch
        self._ctx = C.c_void_p()
        L.check(self._lib.meao_create(C.byref(cfg), C.byref(self._ctx)))

    # ---- the six public properties of the reference (AO.cs:22-66) ----------------------
    def _get(self, name):
        return getattr(self._prm, name)

    def _set(self, name, value):
        if getattr(self._prm, name) != value:   # CheckUpdate (AO.cs:91-102)
            setattr(self._prm, name, value)
            self._dirty = True

    noiseFilterTolerance = property(lambda s: s._get("noise_filter_tolerance"),
                                    lambda s, v: s._set("noise_filter_tolerance", float(v)))
    blurTolerance = property(lambda s: s._get("blur_tolerance"),
                             lambda s, v: s._set("blur_tolerance", float(v)))
    upsampleTolerance = property(lambda s: s._get("upsample_tolerance"),
                                 lambda s, v: s._set("upsample_tolerance", float(v)))
    thicknessModifier = property(lambda s: s._get("thickness_modifier"),
                                 lambda s, v: s._set("thickness_modifier", float(v)))
    intensity = property(lambda s: s._get("intensity"), lambda s, v: s._set("intensity", float(v)))

    @property
    def ambientOnly(self) -> bool:
        return self._ambient_only

    @ambientOnly.setter
    def ambientOnly(self, value: bool) -> None:
        self._ambient_only = bool(value)

    # ---- camera terms Unity supplied implicitly (AO.cs:563-573) ------------------------
    nearClipPlane = property(lambda s: s._get("near_clip"), lambda s, v: s._set("near_clip", float(v)))
    farClipPlane = property(lambda s: s._get("far_clip"), lambda s, v: s._set("far_clip", float(v)))
    projection00 = property(lambda s: s._get("proj00"), lambda s, v: s._set("proj00", float(v)))
    usesReversedZBuffer = property(lambda s: bool(s._get("reversed_z")),
                                   lambda s, v: s._set("reversed_z", 1 if v else 0))
    singlePassStereoEnabled = property(lambda s: bool(s._get("single_pass_stereo")),       # AO.cs:392-401
                                       lambda s, v: s._set("single_pass_stereo", 1 if v else 0))

    # ---- geometry ----------------------------------------------------------------------
    width = property(lambda s: s._cfg.width)
    height = property(lambda s: s._cfg.height)
    ao_format = property(lambda s: s._cfg.ao_format)
    max_batch = property(lambda s: s._cfg.max_batch)
    ao_dtype = property(lambda s: np.uint8 if s._cfg.ao_format == L.AO_R8 else np.uint16)

    def resize(self, width: int, height: int) -> None:
        """Screen-size change (AO.cs:338-341).  Inside a reservation (reserve()) it neither allocates nor synchronises."""
        L.check(self._lib.meao_resize(self._ctx, width, height), self._ctx)
        self._cfg.width, self._cfg.height = width, height
        self._last_sizes = None

    def reserve(self, max_width: int, max_height: int) -> None:
        """Dynamic resolution (meao_reserve): size the intermediates for max_width x max_height once -- it may allocate and
        synchronises the device once; every later resize() to a size inside it moves nothing.  (0, 0) drops the reservation."""
        L.check(self._lib.meao_reserve(self._ctx, max_width, max_height), self._ctx)

    @property
    def capacity(self) -> tuple:
        """The reservation as (width, height); (0, 0) = none (meao_get_capacity)."""
        w, h = C.c_int32(), C.c_int32()
        L.check(self._lib.meao_get_capacity(self._ctx, C.byref(w), C.byref(h)), self._ctx)
        return w.value, h.value

    def reserve_bytes(self, max_width: int, max_height: int) -> int:
        """Device memory a reservation of that size costs this configuration (meao_reserve_bytes; host-plan only)."""
        b = C.c_uint64()
        L.check(self._lib.meao_reserve_bytes(C.byref(self._cfg), max_width, max_height, C.byref(b)))
        return b.value

    def _sync_params(self) -> None:
        if self._dirty:
            L.check(self._lib.meao_set_params(self._ctx, C.byref(self._prm)), self._ctx)
            self._dirty = False

    # ---- the hot path ------------------------------------------------------------------
    def render(self, depth: np.ndarray) -> np.ndarray:
        """One frame, host arrays: (H, W) raw depth in the configured depth_format (float32 by
        default; uint16 / uint32 codes for UNORM16 / UNORM24 / F16 bits; float32 / float16 view-space z for LINEAR_F32 / _F16) -> AO (H, W) uint8 / f16 bits."""
        return self.render_batch([depth])[0]

    def render_batch(self, depths: Sequence[np.ndarray], params: Optional[Sequence[Optional[FrameParams]]] = None) -> list:
        """params: one FrameParams per frame (meao_execute_batch_params; unset fields = this instance's values), or None."""
        n = len(depths)
        self._sync_params()
        self._last_sizes = None
        prm = None if params is None else params_array(params, n, self._prm)
        dt = DEPTH_NUMPY[self._cfg.depth_format]
        ins = [np.ascontiguousarray(d, dtype=dt) for d in depths]
        for d in ins:
            if d.shape != (self.height, self.width):
                raise ValueError(f"depth shape {d.shape} != ({self.height}, {self.width})")
        outs = [np.empty((self.height, self.width), self.ao_dtype) for _ in range(n)]
        pin = (C.c_void_p * n)(*[d.ctypes.data for d in ins])
        pout = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        if prm is None:
            L.check(self._lib.meao_execute_batch(self._ctx, n, pin, L.MEM_HOST, pout, L.MEM_HOST, None), self._ctx)
        else:
            L.check(self._lib.meao_execute_batch_params(self._ctx, n, pin, L.MEM_HOST, pout, L.MEM_HOST, prm, None), self._ctx)
        return outs

    def execute_device(self, depth_ptrs: Sequence[int], out_ptrs: Sequence[int], stream: int = 0,
                       params: Optional[Sequence[Optional[FrameParams]]] = None, *, depth_pitch: int = 0, out_pitch: int = 0,
                       extents: Optional[Sequence[tuple]] = None) -> None:
        """Device-resident frames (raw device addresses, e.g. torch ``data_ptr()``); asynchronous.  params: as in render_batch.
        depth_pitch / out_pitch: bytes between consecutive rows of the surfaces (meao_execute_batch_pitched); 0 = tightly packed.
        extents: one (width, height[, depth_pitch, ao_pitch]) per frame -- a mixed-size batch (meao_execute_batch_extents): every
        size inside the reservation, else inside this context's size; the pitches (bytes, 0 = packed for that frame's width) then
        come from the extents, not from depth_pitch / out_pitch.  debug_buffer / debug_view afterwards have the frame's size."""
        n = len(depth_ptrs)
        self._sync_params()
        pin = (C.c_void_p * n)(*depth_ptrs)
        pout = (C.c_void_p * n)(*out_ptrs)
        s = C.c_void_p(stream) if stream else None
        self._last_sizes = None
        if extents is not None:
            if depth_pitch or out_pitch:
                raise ValueError("execute_device: with extents the pitches are given per frame, inside the extents")
            prm = None if params is None else params_array(params, n, self._prm)
            L.check(self._lib.meao_execute_batch_extents(self._ctx, n, pin, pout, extents_array(extents, n), prm, s), self._ctx)
            self._last_sizes = [(int(e[0]), int(e[1])) for e in extents]
        elif depth_pitch or out_pitch:
            prm = None if params is None else params_array(params, n, self._prm)
            L.check(self._lib.meao_execute_batch_pitched(self._ctx, n, pin, depth_pitch, L.MEM_DEVICE, pout, out_pitch, L.MEM_DEVICE,
                                                         prm, s), self._ctx)
        elif params is None:
            L.check(self._lib.meao_execute_batch(self._ctx, n, pin, L.MEM_DEVICE, pout, L.MEM_DEVICE, s), self._ctx)
        else:
            prm = params_array(params, n, self._prm)
            L.check(self._lib.meao_execute_batch_params(self._ctx, n, pin, L.MEM_DEVICE, pout, L.MEM_DEVICE, prm, s), self._ctx)

    def execute_shaded_device(self, depth_ptrs: Sequence[int], out_ptrs: Sequence[int], mode: int, color_ptrs: Sequence[int],
                              gbuffer0_ptrs: Optional[Sequence[int]] = None, stream: int = 0,
                              params: Optional[Sequence[Optional[FrameParams]]] = None, *, depth_pitch: int = 0, out_pitch: int = 0,
                              color_pitch: int = 0, gbuffer0_pitch: int = 0, color_format: int = L.COLOR_RGBA16F,
                              extents: Optional[Sequence[tuple]] = None, color_pitches: Optional[Sequence[int]] = None,
                              gbuffer0_pitches: Optional[Sequence[int]] = None) -> None:
        """execute_device() followed, on the same stream, by ONE composite launch of out_ptrs[f] into color_ptrs[f]
        (meao_execute_batch_shaded): when the call has completed the colour targets are shaded, whatever their format.  Every
        argument of both halves is checked before anything is enqueued.
        extents: a mixed-size batch as execute_device takes it (meao_execute_batch_extents_shaded); color_pitches /
        gbuffer0_pitches then hold one row pitch in bytes per frame (None = every frame tightly packed) in place of color_pitch /
        gbuffer0_pitch."""
        n = len(depth_ptrs)
        if len(out_ptrs) != n or len(color_ptrs) != n or (gbuffer0_ptrs and len(gbuffer0_ptrs) != n):
            raise ValueError("execute_shaded_device: one AO, one colour (and one GBuffer0) surface per depth frame")
        if extents is None and (color_pitches is not None or gbuffer0_pitches is not None):
            raise ValueError("execute_shaded_device: color_pitches / gbuffer0_pitches go with extents")
        self._sync_params()
        self._last_sizes = None
        prm = None if params is None else params_array(params, n, self._prm)
        g = (C.c_void_p * n)(*gbuffer0_ptrs) if gbuffer0_ptrs else None
        if extents is not None:
            if depth_pitch or out_pitch or color_pitch or gbuffer0_pitch:
                raise ValueError("execute_shaded_device: with extents the pitches are given per frame (extents, color_pitches, gbuffer0_pitches)")
            L.check(self._lib.meao_execute_batch_extents_shaded(
                self._ctx, n, (C.c_void_p * n)(*depth_ptrs), (C.c_void_p * n)(*out_ptrs), extents_array(extents, n), prm, mode,
                (C.c_void_p * n)(*color_ptrs), color_format, _pitch_array(color_pitches, n, "color_pitches"), g,
                _pitch_array(gbuffer0_pitches, n, "gbuffer0_pitches"), C.c_void_p(stream) if stream else None), self._ctx)
            self._last_sizes = [(int(e[0]), int(e[1])) for e in extents]
            return
        L.check(self._lib.meao_execute_batch_shaded(self._ctx, n, (C.c_void_p * n)(*depth_ptrs), depth_pitch, (C.c_void_p * n)(*out_ptrs),
                                                    out_pitch, prm, mode, (C.c_void_p * n)(*color_ptrs), color_format, color_pitch, g,
                                                    gbuffer0_pitch, C.c_void_p(stream) if stream else None), self._ctx)

    def prefetch_device(self, depth_ptrs: Sequence[int], params: Optional[Sequence[Optional[FrameParams]]] = None, *,
                        depth_pitch: int = 0, size: Optional[tuple] = None) -> None:
        """Announce the device depth frames of the call after next (meao_prefetch_batch): the next
        execute_device() carries their downsample pass inside its last upsample kernel.  params: the frames' own
        parameters (meao_prefetch_batch_params), as they will be given to the consuming execute_device().  depth_pitch: their row
        pitch in bytes (meao_prefetch_batch_pitched; 0 = tightly packed), as it will be given to the consuming call.
        size: (width, height) of the announced frames where it is not this context's size -- a size inside the reservation that a
        resize() follows before the consuming call (meao_prefetch_batch_sized)."""
        n = len(depth_ptrs)
        self._sync_params()     # pending property changes first: meao_set_params would drop the announcement
        pin = (C.c_void_p * n)(*depth_ptrs)
        if size is not None:
            prm = None if params is None else params_array(params, n, self._prm)
            L.check(self._lib.meao_prefetch_batch_sized(self._ctx, int(size[0]), int(size[1]), n, pin, depth_pitch, prm), self._ctx)
        elif depth_pitch:
            prm = None if params is None else params_array(params, n, self._prm)
            L.check(self._lib.meao_prefetch_batch_pitched(self._ctx, n, pin, depth_pitch, prm), self._ctx)
        elif params is None:
            L.check(self._lib.meao_prefetch_batch(self._ctx, n, pin), self._ctx)
        else:
            L.check(self._lib.meao_prefetch_batch_params(self._ctx, n, pin, params_array(params, n, self._prm)), self._ctx)

    def execute_tensors(self, depth, out=None, params: Optional[Sequence[Optional[FrameParams]]] = None, *, color=None, gbuffer0=None,
                        mode: int = L.COMPOSITE_MULTIPLY, color_format: int = L.COLOR_RGBA16F):
        """Torch tensors on this context's device, used in place (meao_execute_batch_pitched), on torch.cuda.current_stream().
        depth: an (N, H, W) tensor or a list of (H, W) tensors in the dtype of depth_format (float32, float16, uint16 for UNORM16,
        int32 for UNORM24; float32 / float16 for LINEAR_F32 / LINEAR_F16) -- e.g. a crop ``surface[:, y0:y0 + H, x0:x0 + W]`` of larger targets.  Rows must be contiguous and all
        frames must share one row stride, which becomes the pitch; any other layout raises ValueError (nothing is copied).
        out: the same for the AO (uint8 for R8, float16 for F16 storage), or None: allocated packed.  Returns out.
        color: colour targets as composite_tensors takes them (with gbuffer0, mode and color_format): they are shaded in place by
        the same call (meao_execute_batch_shaded), one composite launch behind the last AO kernel.
        A list of differently shaped (H_f, W_f) tensors is a mixed-size batch (meao_execute_batch_extents, with color
        meao_execute_batch_extents_shaded): out, color and gbuffer0 are then lists of tensors of the frames' sizes, each tensor's own
        row stride becomes its pitch, and the list of AO tensors is returned."""
        import torch
        from .surfaces import frame_pointers, packed_pitch
        depth_dt = getattr(torch, DEPTH_TORCH[self._cfg.depth_format])
        ao_dt = torch.uint8 if self._cfg.ao_format == L.AO_R8 else torch.float16
        dev = torch.device("cuda", self._cfg.device)        # every frame of depth and out must be on the context's device
        frames = list(depth) if not hasattr(depth, "dim") else depth
        if isinstance(frames, list) and any(tuple(t.shape) != (self.height, self.width) for t in frames):
            if gbuffer0 is not None and color is None:
                raise ValueError("execute_tensors: gbuffer0 without color")
            return self._execute_mixed_tensors(frames, out, params, depth_dt, ao_dt, dev, color, gbuffer0, mode, color_format)
        d_ptrs, d_pitch = frame_pointers(frames, self.height, self.width, depth_dt, "depth", device=dev)
        n = len(d_ptrs)
        first = frames[0]
        if out is None:
            out = torch.empty((n, self.height, self.width), dtype=ao_dt, device=dev)
        o_frames = list(out) if not hasattr(out, "dim") else out
        o_ptrs, o_pitch = frame_pointers(o_frames, self.height, self.width, ao_dt, "out", device=dev)
        if len(o_ptrs) != n:
            raise ValueError(f"out has {len(o_ptrs)} frames, depth {n}")
        stream = torch.cuda.current_stream(dev).cuda_stream
        if color is not None:
            from .surfaces import composite_surfaces
            a, ap, c, cp, g, gp = composite_surfaces(out, color, gbuffer0, self.height, self.width, ao_dt, device=dev,
                                                     color_format=color_format)
            if len(c) != n:
                raise ValueError(f"color has {len(c)} frames, depth {n}")
            self.execute_shaded_device(d_ptrs, a, mode, c, g, stream=stream, params=params,
                                       depth_pitch=packed_pitch(d_pitch, self.width, first.element_size()), out_pitch=ap,
                                       color_pitch=cp, gbuffer0_pitch=gp, color_format=color_format)
            return out
        if gbuffer0 is not None:
            raise ValueError("execute_tensors: gbuffer0 without color")
        self.execute_device(d_ptrs, o_ptrs, stream=stream, params=params,
                            depth_pitch=packed_pitch(d_pitch, self.width, first.element_size()),
                            out_pitch=packed_pitch(o_pitch, self.width, o_frames[0].element_size()))
        return out

    def _execute_mixed_tensors(self, frames, out, params, depth_dt, ao_dt, dev, color=None, gbuffer0=None,
                               mode: int = L.COMPOSITE_MULTIPLY, color_format: int = L.COLOR_RGBA16F):
        """execute_tensors for a list of (H_f, W_f) tensors of different shapes (meao_execute_batch_extents): every frame's own
        row stride becomes its pitch.  out: a list of (H_f, W_f) tensors, or None: allocated packed.  Returns the list.
        color (and gbuffer0): lists of the frames' colour (GBuffer0) targets, shaded in place by the same call
        (meao_execute_batch_extents_shaded)."""
        import torch
        from .surfaces import composite_surfaces_per_frame, frame_pointers, packed_pitch
        if out is None:
            out = [torch.empty(tuple(t.shape), dtype=ao_dt, device=dev) for t in frames]
        out = list(out)
        if len(out) != len(frames):
            raise ValueError(f"out has {len(out)} frames, depth {len(frames)}")
        d_ptrs, o_ptrs, extents = [], [], []
        for f, (d, o) in enumerate(zip(frames, out)):
            if d.dim() != 2 or tuple(o.shape) != tuple(d.shape):
                raise ValueError(f"frame {f}: depth {tuple(d.shape)} and out {tuple(o.shape)} must be the same (H, W)")
            h, w = d.shape
            (dp,), d_pitch = frame_pointers([d], h, w, depth_dt, f"depth[{f}]", device=dev)
            (op,), o_pitch = frame_pointers([o], h, w, ao_dt, f"out[{f}]", device=dev)
            d_ptrs.append(dp)
            o_ptrs.append(op)
            extents.append((w, h, packed_pitch(d_pitch, w, d.element_size()), packed_pitch(o_pitch, w, o.element_size())))
        stream = torch.cuda.current_stream(dev).cuda_stream
        if color is not None:
            a, c, g, targets = composite_surfaces_per_frame(out, color, gbuffer0, ao_dt, device=dev, color_format=color_format)
            if len(c) != len(frames):
                raise ValueError(f"color has {len(c)} frames, depth {len(frames)}")
            self.execute_shaded_device(d_ptrs, a, mode, c, g, stream=stream, params=params, color_format=color_format, extents=extents,
                                       color_pitches=[t[3] for t in targets], gbuffer0_pitches=[t[4] for t in targets] if g else None)
            return out
        self.execute_device(d_ptrs, o_ptrs, stream=stream, params=params, extents=extents)
        return out

    def synchronize(self, stream: int = 0) -> None:
        L.check(self._lib.meao_synchronize(self._ctx, C.c_void_p(stream) if stream else None), self._ctx)

    # ---- composite (PushCompositeCommands, AO.cs:822-839) ------------------------------
    # color_format -> (numpy dtype, trailing shape) of a host colour array
    _HOST_COLOR = {L.COLOR_RGBA16F: (np.uint16, (4,)), L.COLOR_RGBA32F: (np.float32, (4,)), L.COLOR_RGBA8: (np.uint8, (4,)),
                   L.COLOR_R11G11B10F: (np.uint32, ()), L.COLOR_RGBA8_SRGB: (np.uint8, (4,))}

    def composite(self, ao: np.ndarray, color_rgba16f: np.ndarray, gbuffer0_rgba8: Optional[np.ndarray] = None,
                  debug: bool = False, color_format: int = L.COLOR_RGBA16F) -> None:
        """Host arrays, in place.  Mode follows the reference: debug view if ``debug`` (AO.cs:826),
        ambient-only into GBuffer0 + the HDR target if ``ambientOnly`` and a GBuffer0 is given
        (AO.cs:830-834), else the standard multiply (AO.cs:837).  color_format: the meao_color_format of the colour array --
        (H, W, 4) uint16 (RGBA16F bits), float32 or uint8, or (H, W) uint32 for R11G11B10F (meao_composite_format)."""
        dt, tail = self._HOST_COLOR[color_format]
        assert color_rgba16f.dtype == dt and color_rgba16f.shape == (self.height, self.width) + tail
        assert ao.dtype == self.ao_dtype and ao.shape == (self.height, self.width)
        if debug:
            mode, g = L.COMPOSITE_DEBUG, None
        elif self._ambient_only and gbuffer0_rgba8 is not None:
            assert gbuffer0_rgba8.dtype == np.uint8 and gbuffer0_rgba8.shape == (self.height, self.width, 4)
            mode, g = L.COMPOSITE_AMBIENT_ONLY, gbuffer0_rgba8.ctypes.data
        else:
            mode, g = L.COMPOSITE_MULTIPLY, None
        if color_format != L.COLOR_RGBA16F:
            L.check(self._lib.meao_composite_format(self._ctx, mode, ao.ctypes.data, 0, color_rgba16f.ctypes.data, color_format, 0, g, 0,
                                                    L.MEM_HOST, None), self._ctx)
            return
        L.check(self._lib.meao_composite(self._ctx, mode, ao.ctypes.data, color_rgba16f.ctypes.data, g,
                                         L.MEM_HOST, None), self._ctx)

    def composite_device(self, mode: int, ao_ptr: int, color_ptr: int, gbuffer0_ptr: int = 0, stream: int = 0, *,
                         ao_pitch: int = 0, color_pitch: int = 0, gbuffer0_pitch: int = 0, color_format: int = L.COLOR_RGBA16F) -> None:
        """ao_pitch / color_pitch / gbuffer0_pitch: bytes between consecutive rows of the surfaces (meao_composite_pitched);
        0 = tightly packed.  color_format: the meao_color_format of the colour surface (meao_composite_format)."""
        s = C.c_void_p(stream) if stream else None
        if color_format != L.COLOR_RGBA16F:
            L.check(self._lib.meao_composite_format(self._ctx, mode, ao_ptr, ao_pitch, color_ptr, color_format, color_pitch,
                                                    gbuffer0_ptr or None, gbuffer0_pitch, L.MEM_DEVICE, s), self._ctx)
        elif ao_pitch or color_pitch or gbuffer0_pitch:
            L.check(self._lib.meao_composite_pitched(self._ctx, mode, ao_ptr, ao_pitch, color_ptr, color_pitch, gbuffer0_ptr or None,
                                                     gbuffer0_pitch, L.MEM_DEVICE, s), self._ctx)
        else:
            L.check(self._lib.meao_composite(self._ctx, mode, ao_ptr, color_ptr, gbuffer0_ptr or None, L.MEM_DEVICE, s), self._ctx)

    def composite_enqueue_device(self, mode: int, ao_ptrs: Sequence[int], color_ptrs: Sequence[int],
                                 gbuffer0_ptrs: Optional[Sequence[int]] = None, *,
                                 ao_pitch: int = 0, color_pitch: int = 0, gbuffer0_pitch: int = 0,
                                 color_format: int = L.COLOR_RGBA16F) -> None:
        """Composite of device frames an earlier execute produced; rides inside the NEXT execute's render
        kernel (meao_composite_enqueue).  composite_flush() runs whatever still waits.  ao_pitch / color_pitch / gbuffer0_pitch:
        row pitches in bytes of every frame's surfaces (meao_composite_enqueue_pitched); 0 = tightly packed.  color_format: the
        meao_color_format of the colour surfaces (meao_composite_enqueue_format); a batch in another format than RGBA16F is run
        by the next execute as launches of its own, in front of its passes."""
        n = len(ao_ptrs)
        g = (C.c_void_p * n)(*gbuffer0_ptrs) if gbuffer0_ptrs else None
        if color_format != L.COLOR_RGBA16F:
            L.check(self._lib.meao_composite_enqueue_format(self._ctx, mode, n, (C.c_void_p * n)(*ao_ptrs), ao_pitch,
                                                            (C.c_void_p * n)(*color_ptrs), color_format, color_pitch, g, gbuffer0_pitch),
                    self._ctx)
        elif ao_pitch or color_pitch or gbuffer0_pitch:
            L.check(self._lib.meao_composite_enqueue_pitched(self._ctx, mode, n, (C.c_void_p * n)(*ao_ptrs), ao_pitch,
                                                             (C.c_void_p * n)(*color_ptrs), color_pitch, g, gbuffer0_pitch), self._ctx)
        else:
            L.check(self._lib.meao_composite_enqueue(self._ctx, mode, n, (C.c_void_p * n)(*ao_ptrs),
                                                     (C.c_void_p * n)(*color_ptrs), g), self._ctx)

    def composite_batch_device(self, mode: int, ao_ptrs: Sequence[int], color_ptrs: Sequence[int],
                               gbuffer0_ptrs: Optional[Sequence[int]] = None, stream: int = 0, *, ao_pitch: int = 0,
                               color_pitch: int = 0, gbuffer0_pitch: int = 0, color_format: int = L.COLOR_RGBA16F,
                               extents: Optional[Sequence[tuple]] = None) -> None:
        """The frames (1..max_batch) composited by ONE launch on ``stream``, now (meao_composite_batch): nothing waits
        afterwards, and a batch that waits from composite_enqueue_device() is left alone.  Arguments as composite_enqueue_device.
        extents: one (width, height[, ao_pitch, color_pitch, gbuffer0_pitch]) per frame -- frames of their own sizes, of any size
        (meao_composite_batch_extents); the pitches (bytes, 0 = packed for that frame's width) then come from the extents."""
        n = len(ao_ptrs)
        g = (C.c_void_p * n)(*gbuffer0_ptrs) if gbuffer0_ptrs else None
        if extents is not None:
            if ao_pitch or color_pitch or gbuffer0_pitch:
                raise ValueError("composite_batch_device: with extents the pitches are given per frame, inside the extents")
            L.check(self._lib.meao_composite_batch_extents(self._ctx, mode, n, (C.c_void_p * n)(*ao_ptrs), (C.c_void_p * n)(*color_ptrs),
                                                           color_format, g, target_extents_array(extents, n),
                                                           C.c_void_p(stream) if stream else None), self._ctx)
            return
        L.check(self._lib.meao_composite_batch(self._ctx, mode, n, (C.c_void_p * n)(*ao_ptrs), ao_pitch, (C.c_void_p * n)(*color_ptrs),
                                               color_format, color_pitch, g, gbuffer0_pitch, C.c_void_p(stream) if stream else None),
                self._ctx)

    def composite_tensors(self, ao, color, gbuffer0=None, mode: int = L.COMPOSITE_MULTIPLY, enqueue: bool = False,
                          color_format: int = L.COLOR_RGBA16F, batched: bool = False) -> None:
        """Torch tensors on this context's device, composited in place (meao_composite_pitched / meao_composite_enqueue_pitched).
        ao: an (N, H, W) tensor or a list of (H, W) in the AO dtype (uint8 for R8, float16 for F16 storage); color: (N, H, W, 4)
        int16 / float16 holding RGBA16F; gbuffer0: (N, H, W, 4) uint8, for COMPOSITE_AMBIENT_ONLY -- e.g. crops
        ``target[:, y0:y0 + H, x0:x0 + W, :]`` of larger targets.  The channels of a texel and the texels of a row must be contiguous
        and all frames of a surface must share one row stride, which becomes its pitch; any other layout raises ValueError
        (nothing is copied).  enqueue=False: one composite per frame now, on torch.cuda.current_stream(); enqueue=True: the
        batch waits for the next execute's render kernel (composite_enqueue_device).  color_format: another meao_color_format
        for ``color`` -- (N, H, W, 4) float32 for RGBA32F or uint8 for RGBA8 / RGBA8_SRGB, (N, H, W) int32 for R11G11B10F.  batched=True (with
        enqueue=False): the frames in one launch now (composite_batch_device) instead of one launch each -- and then ao, color and
        gbuffer0 may be lists of differently shaped frames, each tensor's own row stride becoming its pitch
        (meao_composite_batch_extents)."""
        import torch
        from .surfaces import composite_surfaces, composite_surfaces_per_frame
        ao_dt = torch.uint8 if self._cfg.ao_format == L.AO_R8 else torch.float16
        dev = torch.device("cuda", self._cfg.device)
        if batched and not enqueue and not hasattr(ao, "dim") and any(tuple(t.shape) != (self.height, self.width) for t in ao):
            a, c, g, extents = composite_surfaces_per_frame(ao, color, gbuffer0, ao_dt, device=dev, color_format=color_format)
            self.composite_batch_device(mode, a, c, g, torch.cuda.current_stream(dev).cuda_stream, color_format=color_format, extents=extents)
            return
        a, ap, c, cp, g, gp = composite_surfaces(ao, color, gbuffer0, self.height, self.width, ao_dt, device=dev, color_format=color_format)
        if enqueue:
            if batched:
                raise ValueError("composite_tensors: batched=True composites now; it cannot be combined with enqueue=True")
            self.composite_enqueue_device(mode, a, c, g, ao_pitch=ap, color_pitch=cp, gbuffer0_pitch=gp, color_format=color_format)
            return
        stream = torch.cuda.current_stream(dev).cuda_stream
        if batched:
            self.composite_batch_device(mode, a, c, g, stream, ao_pitch=ap, color_pitch=cp, gbuffer0_pitch=gp, color_format=color_format)
            return
        for f in range(len(a)):
            self.composite_device(mode, a[f], c[f], g[f] if g else 0, stream, ao_pitch=ap, color_pitch=cp, gbuffer0_pitch=gp,
                                  color_format=color_format)

    def composite_flush(self, stream: int = 0) -> None:
        L.check(self._lib.meao_composite_flush(self._ctx, C.c_void_p(stream) if stream else None), self._ctx)

    @property
    def composite_pending(self) -> bool:
        """A batch enqueued with composite_enqueue_device() that no execute / flush / resize has run yet
        (meao_composite_pending: the library's own state, not a mirror of it)."""
        if not self._ctx:
            return False
        n = C.c_int32()
        L.check(self._lib.meao_composite_pending(self._ctx, C.byref(n)), self._ctx)
        return n.value > 0

    # ---- observability (the _debug views, AO.cs:787-820) -------------------------------
    def debug_buffer(self, debug_id: int, frame: int = 0) -> np.ndarray:
        """Debug buffer ``debug_id`` of frame ``frame`` of the last call -- at that frame's own size after a mixed-size batch."""
        d = L.Desc()
        if self._last_sizes is not None and 0 <= frame < len(self._last_sizes):
            cfg = L.Config.from_buffer_copy(self._cfg)
            cfg.width, cfg.height = self._last_sizes[frame]
            L.check(self._lib.meao_describe_buffer(C.byref(cfg), debug_id, C.byref(d)))
        else:
            L.check(self._lib.meao_get_intermediate(self._ctx, frame, debug_id, None, 0, L.MEM_HOST, C.byref(d)), self._ctx)
        shape = (d.slices, d.height, d.width) if d.slices > 1 else (d.height, d.width)
        out = np.empty(shape, _NP_OF_FMT[d.format])
        L.check(self._lib.meao_get_intermediate(self._ctx, frame, debug_id, out.ctypes.data, out.nbytes,
                                                L.MEM_HOST, C.byref(d)), self._ctx)
        return out

    def debug_view(self, debug_id: int, frame: int = 0) -> np.ndarray:
        """What `_debug = debug_id` shows (AO.cs:787-820): the buffer blitted into the AO target."""
        w, h = self.width, self.height
        if self._last_sizes is not None and 0 <= frame < len(self._last_sizes):
            w, h = self._last_sizes[frame]       # a mixed-size batch: the view has the frame's own size
        out = np.empty((h, w), self.ao_dtype)
        L.check(self._lib.meao_debug_view(self._ctx, frame, debug_id, out.ctypes.data, L.MEM_HOST, None), self._ctx)
        return out

    def set_profiling(self, enable) -> None:
        """False / True, or an int N > 1: HIP events around the passes of every Nth execute only (meao_set_profiling)."""
        L.check(self._lib.meao_set_profiling(self._ctx, int(enable)), self._ctx)

    def hostile_frames(self) -> int:
        """Bit mask of the frames of the last execute that ran the IEEE-division bodies (meao_hostile_frames)."""
        m = C.c_uint64()
        L.check(self._lib.meao_hostile_frames(self._ctx, C.byref(m)), self._ctx)
        return m.value

    def debug_set(self, key: int, value: int) -> None:
        """meao_debug_set: launch-structure overrides (identical results)."""
        L.check(self._lib.meao_debug_set(self._ctx, key, value), self._ctx)

    def set_tracing(self, enable: bool) -> None:
        """roctx ranges around every pass (rocprofv3 --marker-trace)."""
        L.check(self._lib.meao_set_tracing(self._ctx, 1 if enable else 0), self._ctx)

    def pass_times_ms(self):
        ms = (C.c_float * L.NUM_PASSES)()
        n = C.c_int32()
        L.check(self._lib.meao_get_pass_times(self._ctx, C.byref(ms), C.byref(n)), self._ctx)
        return list(ms), n.value

    def algorithmic_bytes(self):
        b = (C.c_uint64 * L.NUM_PASSES)()
        L.check(self._lib.meao_algorithmic_bytes(C.byref(self._cfg), C.byref(b)))
        return list(b)

    def selftest(self, which: int) -> int:
        n = C.c_uint64()
        L.check(self._lib.meao_selftest(self._ctx, which, C.byref(n)), self._ctx)
        return n.value

    def close(self, flush_composite: bool = False) -> None:
        """meao_destroy.  A composite batch still waiting is DISCARDED by the library (its targets are caller memory
        that is usually gone when a context dies): pass flush_composite=True while those buffers are alive to run it
        first; otherwise the loss is reported as a RuntimeWarning instead of passing silently."""
        if self._ctx:
            if self.composite_pending:
                if flush_composite:
                    self.composite_flush()
                else:
                    import warnings
                    warnings.warn("AmbientOcclusion.close(): a composite batch was still waiting and is discarded "
                                  "(call composite_flush() or close(flush_composite=True) first)", RuntimeWarning, stacklevel=2)
            self._lib.meao_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AmbientOcclusionPool:
    """One context per device behind the C ABI's meao_pool_*: frame f of a batch runs on member
    f mod G, one host thread, no data-path exchange.  ``devices`` may repeat an ordinal
    (several members on one GPU)."""

    def __init__(self, width: int, height: int, devices: Sequence[int], *, max_batch: int = 1,
                 ao_format: int = L.AO_R8, near_clip: float = 0.3, far_clip: float = 1000.0,
                 projection00: Optional[float] = None, reversed_z: bool = True, intensity: float = 1.0,
                 pipelined: bool = False, depth_format: int = L.DEPTH_F32):
        self._lib = L.load()
        cfg = L.Config()
        self._lib.meao_default_config(C.byref(cfg))
        cfg.width, cfg.height, cfg.max_batch, cfg.ao_format = width, height, max_batch, ao_format
        cfg.depth_format = depth_format     # DEPTH_F32, or linear view-space z: DEPTH_LINEAR_F32 / DEPTH_LINEAR_F16 (float16 arrays)
        cfg.pipelined = 1 if pipelined else 0
        self._cfg = cfg
        self.devices = list(devices)
        self._pool = C.c_void_p()
        arr = (C.c_int32 * len(self.devices))(*self.devices)
        status = self._lib.meao_pool_create(C.byref(cfg), arr, len(self.devices), C.byref(self._pool))
        if status != L.OK:
            raise L.MeaoError(status, self._lib.meao_pool_last_error(None).decode())
        prm = L.Params()
        self._lib.meao_default_params(C.byref(prm))
        prm.near_clip, prm.far_clip, prm.reversed_z, prm.intensity = near_clip, far_clip, 1 if reversed_z else 0, intensity
        if projection00 is not None:
            prm.proj00 = projection00
        self._prm = prm           # what unset FrameParams fields take
        try:
            self._check(self._lib.meao_pool_set_params(self._pool, C.byref(prm)))
        except Exception:
            self.close()        # the pool exists already: do not leak its contexts
            raise

    def _check(self, status: int) -> None:
        if status != L.OK:
            raise L.MeaoError(status, self._lib.meao_pool_last_error(self._pool).decode())

    size = property(lambda s: s._lib.meao_pool_size(s._pool))

    def device_of_frame(self, frame: int) -> int:
        return self._lib.meao_pool_device_of_frame(self._pool, frame)

    def render_batch(self, depths: Sequence[np.ndarray], params: Optional[Sequence[Optional[FrameParams]]] = None) -> list:
        """Host arrays in and out.  params: one FrameParams per frame (it goes with the frame to its member), or None."""
        n = len(depths)
        ins = [np.ascontiguousarray(d, dtype=DEPTH_NUMPY[self._cfg.depth_format]) for d in depths]
        dt = np.uint8 if self._cfg.ao_format == L.AO_R8 else np.uint16
        outs = [np.empty((self._cfg.height, self._cfg.width), dt) for _ in range(n)]
        pin = (C.c_void_p * n)(*[d.ctypes.data for d in ins])
        pout = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        if params is None:
            self._check(self._lib.meao_pool_execute_batch(self._pool, n, pin, L.MEM_HOST, pout, L.MEM_HOST))
        else:
            self._check(self._lib.meao_pool_execute_batch_params(self._pool, n, pin, L.MEM_HOST, pout, L.MEM_HOST,
                                                                 params_array(params, n, self._prm)))
        return outs

    def execute_device(self, depth_ptrs: Sequence[int], out_ptrs: Sequence[int],
                       params: Optional[Sequence[Optional[FrameParams]]] = None, *, depth_pitch: int = 0, out_pitch: int = 0,
                       extents: Optional[Sequence[tuple]] = None) -> None:
        """Frame f resident on device_of_frame(f); asynchronous (synchronize()).  depth_pitch / out_pitch: row pitches in bytes of
        every frame's surfaces (meao_pool_execute_batch_pitched); 0 = tightly packed.  extents: a mixed-size batch, as
        AmbientOcclusion.execute_device takes it (meao_pool_execute_batch_extents); extents[f] goes with frame f to its member."""
        n = len(depth_ptrs)
        pin, pout = (C.c_void_p * n)(*depth_ptrs), (C.c_void_p * n)(*out_ptrs)
        if extents is not None:
            if depth_pitch or out_pitch:
                raise ValueError("execute_device: with extents the pitches are given per frame, inside the extents")
            prm = None if params is None else params_array(params, n, self._prm)
            self._check(self._lib.meao_pool_execute_batch_extents(self._pool, n, pin, pout, extents_array(extents, n), prm))
        elif depth_pitch or out_pitch:
            prm = None if params is None else params_array(params, n, self._prm)
            self._check(self._lib.meao_pool_execute_batch_pitched(self._pool, n, pin, depth_pitch, L.MEM_DEVICE, pout, out_pitch,
                                                                  L.MEM_DEVICE, prm))
        elif params is None:
            self._check(self._lib.meao_pool_execute_batch(self._pool, n, pin, L.MEM_DEVICE, pout, L.MEM_DEVICE))
        else:
            self._check(self._lib.meao_pool_execute_batch_params(self._pool, n, pin, L.MEM_DEVICE, pout, L.MEM_DEVICE,
                                                                 params_array(params, n, self._prm)))

    def execute_shaded_device(self, depth_ptrs: Sequence[int], out_ptrs: Sequence[int], mode: int, color_ptrs: Sequence[int],
                              gbuffer0_ptrs: Optional[Sequence[int]] = None,
                              params: Optional[Sequence[Optional[FrameParams]]] = None, *, depth_pitch: int = 0, out_pitch: int = 0,
                              color_pitch: int = 0, gbuffer0_pitch: int = 0, color_format: int = L.COLOR_RGBA16F,
                              extents: Optional[Sequence[tuple]] = None, color_pitches: Optional[Sequence[int]] = None,
                              gbuffer0_pitches: Optional[Sequence[int]] = None) -> None:
        """AmbientOcclusion.execute_shaded_device for the pool (meao_pool_execute_batch_shaded): frame f resident on
        device_of_frame(f); each member runs its execute and one batched composite launch.  Asynchronous (synchronize()).
        extents, color_pitches, gbuffer0_pitches: a mixed-size batch, as AmbientOcclusion.execute_shaded_device takes it
        (meao_pool_execute_batch_extents_shaded); frame f's entries go with it to its member."""
        n = len(depth_ptrs)
        if len(out_ptrs) != n or len(color_ptrs) != n or (gbuffer0_ptrs and len(gbuffer0_ptrs) != n):
            raise ValueError("execute_shaded_device: one AO, one colour (and one GBuffer0) surface per depth frame")
        if extents is None and (color_pitches is not None or gbuffer0_pitches is not None):
            raise ValueError("execute_shaded_device: color_pitches / gbuffer0_pitches go with extents")
        prm = None if params is None else params_array(params, n, self._prm)
        g = (C.c_void_p * n)(*gbuffer0_ptrs) if gbuffer0_ptrs else None
        if extents is not None:
            if depth_pitch or out_pitch or color_pitch or gbuffer0_pitch:
                raise ValueError("execute_shaded_device: with extents the pitches are given per frame (extents, color_pitches, gbuffer0_pitches)")
            self._check(self._lib.meao_pool_execute_batch_extents_shaded(
                self._pool, n, (C.c_void_p * n)(*depth_ptrs), (C.c_void_p * n)(*out_ptrs), extents_array(extents, n), prm, mode,
                (C.c_void_p * n)(*color_ptrs), color_format, _pitch_array(color_pitches, n, "color_pitches"), g,
                _pitch_array(gbuffer0_pitches, n, "gbuffer0_pitches")))
            return
        self._check(self._lib.meao_pool_execute_batch_shaded(self._pool, n, (C.c_void_p * n)(*depth_ptrs), depth_pitch,
                                                             (C.c_void_p * n)(*out_ptrs), out_pitch, prm, mode,
                                                             (C.c_void_p * n)(*color_ptrs), color_format, color_pitch, g, gbuffer0_pitch))

    def reserve(self, max_width: int, max_height: int) -> None:
        """meao_pool_reserve: AmbientOcclusion.reserve for every member."""
        self._check(self._lib.meao_pool_reserve(self._pool, max_width, max_height))

    def resize(self, width: int, height: int) -> None:
        """meao_pool_resize: a size every member's reservation covers (reserve() first); no allocation, no synchronisation."""
        self._check(self._lib.meao_pool_resize(self._pool, width, height))
        self._cfg.width, self._cfg.height = width, height

    def prefetch_device(self, depth_ptrs: Sequence[int], params: Optional[Sequence[Optional[FrameParams]]] = None, *,
                        depth_pitch: int = 0, size: Optional[tuple] = None) -> None:
        """meao_pool_prefetch_batch: the frames of the call after next, dealt like execute_device deals them.  depth_pitch: their
        row pitch in bytes (meao_pool_prefetch_batch_pitched; 0 = tightly packed).  size: (width, height) of the announced frames
        where a resize() follows before the consuming call (meao_pool_prefetch_batch_sized)."""
        n = len(depth_ptrs)
        if size is not None:
            prm = None if params is None else params_array(params, n, self._prm)
            self._check(self._lib.meao_pool_prefetch_batch_sized(self._pool, int(size[0]), int(size[1]), n, (C.c_void_p * n)(*depth_ptrs),
                                                                 depth_pitch, prm))
        elif depth_pitch:
            prm = None if params is None else params_array(params, n, self._prm)
            self._check(self._lib.meao_pool_prefetch_batch_pitched(self._pool, n, (C.c_void_p * n)(*depth_ptrs), depth_pitch, prm))
        elif params is None:
            self._check(self._lib.meao_pool_prefetch_batch(self._pool, n, (C.c_void_p * n)(*depth_ptrs)))
        else:
            self._check(self._lib.meao_pool_prefetch_batch_params(self._pool, n, (C.c_void_p * n)(*depth_ptrs),
                                                                  params_array(params, n, self._prm)))

    def composite_enqueue_device(self, mode: int, ao_ptrs: Sequence[int], color_ptrs: Sequence[int],
                                 gbuffer0_ptrs: Optional[Sequence[int]] = None, *,
                                 ao_pitch: int = 0, color_pitch: int = 0, gbuffer0_pitch: int = 0,
                                 color_format: int = L.COLOR_RGBA16F) -> None:
        """ao_pitch / color_pitch / gbuffer0_pitch: row pitches in bytes of every frame's surfaces
        (meao_pool_composite_enqueue_pitched); 0 = tightly packed.  color_format: the meao_color_format of the colour surfaces
        (meao_pool_composite_enqueue_format)."""
        n = len(ao_ptrs)
        g = (C.c_void_p * n)(*gbuffer0_ptrs) if gbuffer0_ptrs else None
        if color_format != L.COLOR_RGBA16F:
            self._check(self._lib.meao_pool_composite_enqueue_format(self._pool, mode, n, (C.c_void_p * n)(*ao_ptrs), ao_pitch,
                                                                     (C.c_void_p * n)(*color_ptrs), color_format, color_pitch, g,
                                                                     gbuffer0_pitch))
        elif ao_pitch or color_pitch or gbuffer0_pitch:
            self._check(self._lib.meao_pool_composite_enqueue_pitched(self._pool, mode, n, (C.c_void_p * n)(*ao_ptrs), ao_pitch,
                                                                      (C.c_void_p * n)(*color_ptrs), color_pitch, g, gbuffer0_pitch))
        else:
            self._check(self._lib.meao_pool_composite_enqueue(self._pool, mode, n, (C.c_void_p * n)(*ao_ptrs),
                                                              (C.c_void_p * n)(*color_ptrs), g))

    def composite_tensors(self, ao, color, gbuffer0=None, mode: int = L.COMPOSITE_MULTIPLY, enqueue: bool = True,
                          color_format: int = L.COLOR_RGBA16F) -> None:
        """AmbientOcclusion.composite_tensors for the pool, frame f resident on device_of_frame(f).  The pool composites only
        through its members' next calls: enqueue must stay True."""
        import torch
        from .surfaces import composite_surfaces
        if not enqueue:
            raise ValueError("AmbientOcclusionPool.composite_tensors: the pool has no stand-alone composite (enqueue=True)")
        ao_dt = torch.uint8 if self._cfg.ao_format == L.AO_R8 else torch.float16
        a, ap, c, cp, g, gp = composite_surfaces(ao, color, gbuffer0, self._cfg.height, self._cfg.width, ao_dt, color_format=color_format)
        self.composite_enqueue_device(mode, a, c, g, ao_pitch=ap, color_pitch=cp, gbuffer0_pitch=gp, color_format=color_format)

    def composite_flush(self) -> None:
        self._check(self._lib.meao_pool_composite_flush(self._pool))

    @property
    def composite_pending(self) -> bool:
        """Frames of an enqueued composite batch still waiting in any member (meao_pool_composite_pending)."""
        if not self._pool:
            return False
        n = C.c_int32()
        self._check(self._lib.meao_pool_composite_pending(self._pool, C.byref(n)))
        return n.value > 0

    def configure(self, key: int, value: int) -> None:
        """meao_pool_configure: L.POOL_SPIN_US (how long a worker spins for its next job), L.POOL_BIND_NUMA (workers bind to their
        device's NUMA node; before the first DEVICE batch)."""
        self._check(self._lib.meao_pool_configure(self._pool, key, value))

    def member_placement(self, member: int) -> dict:
        """{"numa_node": node of the member's device (-1 unknown), "worker_bound": its worker thread runs on that node}."""
        node, bound = C.c_int32(), C.c_int32()
        self._check(self._lib.meao_pool_member_placement(self._pool, member, C.byref(node), C.byref(bound)))
        return {"numa_node": node.value, "worker_bound": bool(bound.value)}

    def gather_path(self, member: int, dst_device: int) -> int:
        """L.POOL_PATH_*: how gather_to_device copies from `member`'s device to dst_device."""
        return self._lib.meao_pool_gather_path(self._pool, member, dst_device)

    def member_context(self, member: int):
        """Raw meao_ctx* of a member (owned by the pool), e.g. for meao_set_profiling / meao_get_pass_times."""
        return C.c_void_p(self._lib.meao_pool_context(self._pool, member))

    def gather_to_device(self, src_ptrs: Sequence[int], dst_ptrs: Sequence[int], dst_device: int) -> None:
        n = len(src_ptrs)
        self._check(self._lib.meao_pool_gather_to_device(self._pool, n, (C.c_void_p * n)(*src_ptrs),
                                                         (C.c_void_p * n)(*dst_ptrs), dst_device))

    def synchronize(self) -> None:
        self._check(self._lib.meao_pool_synchronize(self._pool))

    def close(self, flush_composite: bool = False) -> None:
        """meao_pool_destroy; a composite still waiting is discarded unless flush_composite (see AmbientOcclusion.close)."""
        if self._pool:
            if self.composite_pending:
                if flush_composite:
                    self.composite_flush()
                else:
                    import warnings
                    warnings.warn("AmbientOcclusionPool.close(): a composite batch was still waiting and is discarded "
                                  "(call composite_flush() or close(flush_composite=True) first)", RuntimeWarning, stacklevel=2)
            self._lib.meao_pool_destroy(self._pool)
            self._pool = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
