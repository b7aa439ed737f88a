"""Row-pitched surfaces (meao_execute_batch_pitched): frames as (pointer, row pitch) pairs.

``frame_pointers`` turns an (N, H, W) tensor, or a list of (H, W) tensors, into the per-frame addresses and the one row pitch in
bytes the C ABI takes.  A crop ``depth[:, y0:y1, x0:x1]`` of a larger surface, a batch slice or a stack of viewports are all
accepted as they are: rows must be contiguous (``stride(-1) == 1``) and every frame must have the same row stride.  Nothing is
ever copied: another layout raises ValueError.  Works on tensors of any device (the addresses are what the caller passes on).

Surfaces with a trailing channel dimension (the composite's RGBA16F colour and RGBA8 GBuffer0 targets, ``channels=4``) are
(N, H, W, C) tensors or lists of (H, W, C): the channels of a texel and the texels of a row must be contiguous.
``composite_surfaces`` gathers the three surfaces of ``composite_tensors``.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple


def frame_pointers(frames, height: int, width: int, dtype, what: str = "depth", device=None, channels: int = 0) -> Tuple[List[int], int]:
    """-> ([data address of frame f], row pitch in bytes).  ``frames``: an (N, H, W) tensor or a sequence of (H, W) tensors, each
    of ``dtype`` (one dtype or a tuple of accepted ones) and of shape (height, width) -- and, if ``device`` is given, on that
    device.  ``channels`` > 0: (N, H, W, channels) / (H, W, channels) instead, a texel being ``channels`` contiguous elements."""
    if channels:
        return _channel_frame_pointers(frames, height, width, dtype, what, device, channels)
    if hasattr(frames, "dim"):
        if frames.dim() != 3:
            raise ValueError(f"{what}: expected an (N, H, W) tensor or a list of (H, W) tensors, got shape {tuple(frames.shape)}")
        seq: Sequence = frames.unbind(0)
    else:
        seq = list(frames)
    if len(seq) == 0:
        raise ValueError(f"{what}: no frames")
    ptrs, row_stride = [], None
    for f, t in enumerate(seq):
        if t.dtype != dtype:
            raise ValueError(f"{what}[{f}]: dtype {t.dtype}, the context expects {dtype}")
        if device is not None and t.device != device:
            raise ValueError(f"{what}[{f}]: on {t.device}, expected {device}")
        if tuple(t.shape) != (height, width):
            raise ValueError(f"{what}[{f}]: shape {tuple(t.shape)} != ({height}, {width})")
        if t.stride(-1) != 1 and width > 1:
            raise ValueError(f"{what}[{f}]: texels of a row are not contiguous (stride(-1) = {t.stride(-1)})")
        rs = t.stride(-2) if height > 1 else width
        if rs < width:
            raise ValueError(f"{what}[{f}]: rows overlap (stride(-2) = {rs} < width {width})")
        if row_stride is None:
            row_stride = rs
        elif rs != row_stride:
            raise ValueError(f"{what}: frames have different row strides ({row_stride} and {rs}); one pitch per call")
        ptrs.append(t.data_ptr())
    return ptrs, row_stride * seq[0].element_size()


def _channel_frame_pointers(frames, height, width, dtype, what, device, channels) -> Tuple[List[int], int]:
    dtypes = tuple(dtype) if isinstance(dtype, (tuple, list)) else (dtype,)
    if hasattr(frames, "dim"):
        if frames.dim() != 4:
            raise ValueError(f"{what}: expected an (N, H, W, {channels}) tensor or a list of (H, W, {channels}) tensors, "
                             f"got shape {tuple(frames.shape)}")
        seq: Sequence = frames.unbind(0)
    else:
        seq = list(frames)
    if len(seq) == 0:
        raise ValueError(f"{what}: no frames")
    ptrs, row_stride = [], None
    for f, t in enumerate(seq):
        if t.dtype not in dtypes:
            raise ValueError(f"{what}[{f}]: dtype {t.dtype}, expected one of {dtypes}")
        if device is not None and t.device != device:
            raise ValueError(f"{what}[{f}]: on {t.device}, expected {device}")
        if tuple(t.shape) != (height, width, channels):
            raise ValueError(f"{what}[{f}]: shape {tuple(t.shape)} != ({height}, {width}, {channels})")
        if t.stride(-1) != 1:
            raise ValueError(f"{what}[{f}]: the channels of a texel are not contiguous (stride(-1) = {t.stride(-1)})")
        if t.stride(-2) != channels and width > 1:
            raise ValueError(f"{what}[{f}]: texels of a row are not contiguous (stride(-2) = {t.stride(-2)})")
        rs = t.stride(-3) if height > 1 else width * channels
        if rs < width * channels:
            raise ValueError(f"{what}[{f}]: rows overlap (stride(-3) = {rs} < width x channels {width * channels})")
        if row_stride is None:
            row_stride = rs
        elif rs != row_stride:
            raise ValueError(f"{what}: frames have different row strides ({row_stride} and {rs}); one pitch per call")
        ptrs.append(t.data_ptr())
    return ptrs, row_stride * seq[0].element_size()


def color_layout(color_format: int):
    """meao_color_format -> (accepted torch dtypes, channels of the tensor's last dimension or 0 for none, bytes per texel):
    RGBA16F (N, H, W, 4) float16 / int16, RGBA32F (N, H, W, 4) float32, RGBA8 and RGBA8_SRGB (N, H, W, 4) uint8, R11G11B10F (N, H, W) int32."""
    import torch
    layouts = {0: ((torch.float16, torch.int16), 4, 8), 1: ((torch.float32,), 4, 16), 2: ((torch.uint8,), 4, 4), 3: ((torch.int32,), 0, 4),
               5: ((torch.uint8,), 4, 4)}
    if color_format not in layouts:
        raise ValueError(f"color_format {color_format}: not a meao_color_format")
    return layouts[color_format]


def composite_surfaces(ao, color, gbuffer0, height: int, width: int, ao_dtype, device=None, color_format: int = 0):
    """The surfaces of ``composite_tensors`` -> (ao_ptrs, ao_pitch, color_ptrs, color_pitch, gbuffer0_ptrs | None, gbuffer0_pitch),
    pitches as the C ABI takes them (0 where tightly packed).  ao: (N, H, W) / list of (H, W) in ``ao_dtype``; color: (N, H, W, 4)
    int16 / float16 (RGBA16F bits) -- or, where ``color_format`` names another meao_color_format, that format's layout and nothing
    else (``color_layout``); gbuffer0: (N, H, W, 4) uint8 or None.  The same frame count everywhere."""
    import torch
    color_dt, color_channels, color_elem = color_layout(color_format)
    a_ptrs, a_pitch = frame_pointers(ao, height, width, ao_dtype, "ao", device=device)
    if color_channels:
        c_ptrs, c_pitch = frame_pointers(color, height, width, color_dt, "color", device=device, channels=color_channels)
    else:
        c_ptrs, c_pitch = frame_pointers(color, height, width, color_dt[0], "color", device=device)
    if len(c_ptrs) != len(a_ptrs):
        raise ValueError(f"color has {len(c_ptrs)} frames, ao {len(a_ptrs)}")
    g_ptrs, g_pitch = None, 0
    if gbuffer0 is not None:
        g_ptrs, g_pitch = frame_pointers(gbuffer0, height, width, torch.uint8, "gbuffer0", device=device, channels=4)
        if len(g_ptrs) != len(a_ptrs):
            raise ValueError(f"gbuffer0 has {len(g_ptrs)} frames, ao {len(a_ptrs)}")
        g_pitch = packed_pitch(g_pitch, width, 4)
    ao_elem = (ao[0] if not hasattr(ao, "dim") else ao).element_size()
    return a_ptrs, packed_pitch(a_pitch, width, ao_elem), c_ptrs, packed_pitch(c_pitch, width, color_elem), g_ptrs, g_pitch


def composite_surfaces_per_frame(ao, color, gbuffer0, ao_dtype, device=None, color_format: int = 0):
    """``composite_surfaces`` for lists of differently shaped frames (meao_composite_batch_extents): frame f is ao[f] of shape
    (H_f, W_f), color[f] and, if given, gbuffer0[f] of that size, and each tensor's own row stride becomes its pitch.
    -> (ao_ptrs, color_ptrs, gbuffer0_ptrs | None, [(W_f, H_f, ao_pitch, color_pitch, gbuffer0_pitch)])."""
    ao, color = list(ao), list(color)
    gbuffer0 = None if gbuffer0 is None else list(gbuffer0)
    if len(color) != len(ao):
        raise ValueError(f"color has {len(color)} frames, ao {len(ao)}")
    if gbuffer0 is not None and len(gbuffer0) != len(ao):
        raise ValueError(f"gbuffer0 has {len(gbuffer0)} frames, ao {len(ao)}")
    a_ptrs, c_ptrs, g_ptrs, extents = [], [], None if gbuffer0 is None else [], []
    for f, a in enumerate(ao):
        if a.dim() != 2:
            raise ValueError(f"ao[{f}]: expected an (H, W) tensor, got shape {tuple(a.shape)}")
        h, w = a.shape
        (ap,), a_pitch, (cp,), c_pitch, g, g_pitch = composite_surfaces([a], [color[f]], None if gbuffer0 is None else [gbuffer0[f]],
                                                                        h, w, ao_dtype, device=device, color_format=color_format)
        a_ptrs.append(ap)
        c_ptrs.append(cp)
        if g_ptrs is not None:
            g_ptrs.append(g[0])
        extents.append((w, h, a_pitch, c_pitch, g_pitch))
    return a_ptrs, c_ptrs, g_ptrs, extents


def packed_pitch(pitch: int, width: int, element_size: int) -> int:
    """The pitch the C ABI is given: 0 where the rows are tightly packed (the same kernels either way)."""
    return 0 if pitch == width * element_size else pitch

