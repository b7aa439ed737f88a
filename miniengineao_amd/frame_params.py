"""Per-frame camera and AO parameters for batched execution (meao_execute_batch_params).

A ``FrameParams`` carries the instance's property names; a field left as None takes the instance's
current value when the batch is submitted.  ``to_params`` turns one into the C ``meao_params`` block.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import Optional, Sequence

from . import _lib as L

# FrameParams field -> meao_params field
_C_FIELD = {
    "nearClipPlane": "near_clip", "farClipPlane": "far_clip", "projection00": "proj00",
    "usesReversedZBuffer": "reversed_z", "singlePassStereoEnabled": "single_pass_stereo",
    "intensity": "intensity", "thicknessModifier": "thickness_modifier",
    "noiseFilterTolerance": "noise_filter_tolerance", "blurTolerance": "blur_tolerance",
    "upsampleTolerance": "upsample_tolerance",
}
_BOOL = ("usesReversedZBuffer", "singlePassStereoEnabled")


@dataclass
class FrameParams:
    """One frame's camera and AO properties; None = the instance's current value."""
    nearClipPlane: Optional[float] = None
    farClipPlane: Optional[float] = None
    projection00: Optional[float] = None
    usesReversedZBuffer: Optional[bool] = None
    singlePassStereoEnabled: Optional[bool] = None
    intensity: Optional[float] = None
    thicknessModifier: Optional[float] = None
    noiseFilterTolerance: Optional[float] = None
    blurTolerance: Optional[float] = None
    upsampleTolerance: Optional[float] = None


def to_params(fp: FrameParams, base: L.Params) -> L.Params:
    """``base`` (the instance's meao_params) with the fields ``fp`` sets replaced."""
    out = L.Params()
    C.memmove(C.byref(out), C.byref(base), C.sizeof(L.Params))      # struct_size and every unset field from the instance
    for f in fields(FrameParams):
        v = getattr(fp, f.name)
        if v is None:
            continue
        setattr(out, _C_FIELD[f.name], (1 if v else 0) if f.name in _BOOL else float(v))
    return out


def params_array(frame_params: Sequence[Optional[FrameParams]], n: int, base: L.Params):
    """A ctypes array of n meao_params, one per frame (an entry of None = the instance's parameters)."""
    if len(frame_params) != n:
        raise ValueError(f"params: {len(frame_params)} entries for {n} frames (one per frame)")
    arr = (L.Params * n)()
    for i, fp in enumerate(frame_params):
        arr[i] = to_params(fp if fp is not None else FrameParams(), base)
    return arr
