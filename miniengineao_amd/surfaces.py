"""Row-pitched surfaces (meao_execute_batch_pitched): frames as (pointer, row pitch) pairs.

``frame_pointers`` turns an (N, H, W) tensor, or a list of (H, W) tensors, into the per-frame addresses and the one row pitch in
bytes the C ABI takes.  A crop ``depth[:, y0:y1, x0:x1]`` of a larger surface, a batch slice or a stack of viewports are all
accepted as they are: rows must be contiguous (``stride(-1) == 1``) and every frame must have the same row stride.  Nothing is
ever copied: another layout raises ValueError.  Works on tensors of any device (the addresses are what the caller passes on).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple


def frame_pointers(frames, height: int, width: int, dtype, what: str = "depth", device=None) -> Tuple[List[int], int]:
    """-> ([data address of frame f], row pitch in bytes).  ``frames``: an (N, H, W) tensor or a sequence of (H, W) tensors, each
    of ``dtype`` and of shape (height, width) -- and, if ``device`` is given, on that device."""
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


def packed_pitch(pitch: int, width: int, element_size: int) -> int:
    """The pitch the C ABI is given: 0 where the rows are tightly packed (the same kernels either way)."""
    return 0 if pitch == width * element_size else pitch

