"""FrameStream: an iterable of depth frames in, an iterable of AO frames out, at the rate of the pipelined step.

The library's fastest form is the pipelined loop of include/meao.h: announce the frames of step k+1 (meao_prefetch_batch*), execute
step k -- its last kernel carries their downsample pass -- then execute step k+1 with exactly the announced pointers, pitch,
Z parameters and stream, a resize in between where the size changes (meao_prefetch_batch_sized inside a reservation).
``FrameStream`` drives that loop for frames that arrive one by one, on the host (NumPy arrays) or on the device (torch tensors),
of one size or of sizes that change inside ``max_size``, with or without per-frame cameras.  The order of the calls is
``stream_plan.Planner``'s; this module executes it.  It adds no kernel: the hot path is the library's kernels, driven without
stalls.

Streams.  The compute stream is ``torch.cuda.current_stream(device)`` at ``run``.  Host frames are copied into pinned slots and
uploaded on one copy stream into three device depth slots; results are downloaded on a second copy stream from two device result
slots into pinned slots; the three streams are tied by events.  In steady state the host waits on two events only -- the upload
of the step it is about to announce and the download of the step it is about to yield -- and never synchronises the compute
stream or the context.  Device frames are used in place: the stream holds a reference to each input tensor until its result has
been yielded, and the caller keeps its contents unchanged until then (the rule of meao_prefetch_batch).  A device result is a
fresh tensor from torch's allocator, ordered on the compute stream: no host wait is needed to use it there.

Camera properties are fixed for the lifetime of a ``run`` (setting one on ``.ao`` meanwhile raises: it would silently drop the
announcement); per-frame cameras go through ``(frame, FrameParams)``.

Out of scope: the pool (its member streams cannot be reached through the ABI), shaded output (the composite), and a C++ or C#
counterpart of this class.
"""
from __future__ import annotations

from typing import Iterable, Iterator, Optional, Tuple

import numpy as np

from . import _lib as L
from . import stream_plan as P
from .ambient_occlusion import DEPTH_NUMPY, DEPTH_TORCH, AmbientOcclusion
from .frame_params import FrameParams
from .surfaces import packed_pitch

_ALIGN = 256                # bytes: every frame of a slot starts aligned, so the 4-texel vector forms stay eligible
_LEGACY_STREAM = 1          # hipStreamLegacy: the null stream by a non-zero handle (0 would select the context's own stream)


def _aligned(nbytes: int) -> int:
    return (nbytes + _ALIGN - 1) // _ALIGN * _ALIGN


class _StreamAO(AmbientOcclusion):
    """The stream's context: property changes are refused while a run is active."""
    _run = None

    def _set(self, name, value):
        if self._run is not None and getattr(self._prm, name) != value:
            raise ValueError(f"AmbientOcclusion.{name} cannot change while FrameStream.run is active (frame {self._run.frames_out} is "
                             "the next to be yielded): it would drop the announced step; use (frame, FrameParams) for per-frame values")
        super()._set(name, value)


class _Slots:
    """`count` device buffers and as many pinned host buffers of `nbytes`, allocated once."""

    def __init__(self, torch, count: int, nbytes: int, device):
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=device) for _ in range(count)]
        self.pin = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(count)]
        self.host = [p.numpy() for p in self.pin]          # the same memory, for the host-side copies
        self.free_after = [None] * count                   # event behind the last device work that read or wrote dev[slot]


class _Run:
    def __init__(self):
        self.frames_out = 0


class FrameStream:
    """FrameStream(width, height, *, batch=16, max_size=None, device=0, **ambient_occlusion_kwargs)

    ``run(frames)`` yields one AO frame per input frame, in input order.  ``frames``: an iterable of (H, W) NumPy arrays or torch
    tensors on the context's device in the dtype of ``depth_format`` (ambient_occlusion.DEPTH_NUMPY / DEPTH_TORCH), or of
    ``(frame, FrameParams)`` pairs.  A NumPy frame yields a fresh NumPy array the caller owns, a tensor yields a fresh tensor
    (float16 for F16 storage).  Rows must be contiguous; a tensor may have a row stride (a crop of a wider surface).
    ``max_size=(W, H)`` reserves room once for frames of any size up to it (AmbientOcclusion.reserve); without it every frame
    has the construction size.  At most ``batch`` frames go into one call; the input is read at most two steps ahead of what
    has been yielded (stream_plan).  A frame that cannot be taken raises ValueError naming its index, after the results of all
    frames in front of it have been yielded.
    ``stats``: steps, frames, announced, sized_announcements, resizes -- summed over the runs.
    Out of scope: the pool, shaded output, a C++ or C# counterpart (module docstring)."""

    def __init__(self, width: int, height: int, *, batch: int = 16, max_size: Optional[Tuple[int, int]] = None, device: int = 0,
                 **ambient_occlusion_kwargs):
        import torch
        self._torch = torch
        self.batch = int(batch)
        self.ao = _StreamAO(width, height, device=device, max_batch=self.batch, pipelined=True, **ambient_occlusion_kwargs)
        try:
            self._reserved = max_size is not None
            if self._reserved:
                self.ao.reserve(int(max_size[0]), int(max_size[1]))
            self.capacity = (int(max_size[0]), int(max_size[1])) if self._reserved else (width, height)
        except Exception:
            self.ao.close()
            raise
        self._device = torch.device("cuda", device)
        fmt = self.ao._cfg.depth_format
        self._np_depth, self._torch_depth = np.dtype(DEPTH_NUMPY[fmt]), getattr(torch, DEPTH_TORCH[fmt])
        self._np_ao = np.dtype(self.ao.ao_dtype)
        self._torch_ao = torch.uint8 if self.ao.ao_format == L.AO_R8 else torch.float16
        self._depth_slots = self._result_slots = None       # allocated at the first host frame, for the capacity
        self._upload = self._download = None
        self._stats = dict(steps=0, frames=0, announced=0, sized_announcements=0, resizes=0)
        self._active = False

    # ---- public surface ----------------------------------------------------------------
    @property
    def stats(self) -> dict:
        return dict(self._stats)

    def close(self) -> None:
        if self.ao is not None and self.ao._ctx:
            self.ao._run = None
            self.ao.close()
        self._depth_slots = self._result_slots = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def run(self, frames: Iterable) -> Iterator:
        """The results of ``frames``, lazily: nothing is read or submitted before the first next()."""
        return self._run_generator(frames)

    # ---- the frames --------------------------------------------------------------------
    def _describe(self, frames: Iterable, store: dict) -> Iterator[tuple]:
        """stream_plan's metadata of every frame, lazily; the frame itself goes into `store`.  A frame that cannot be taken
        raises ValueError, which the planner defers until everything in front of it has been yielded."""
        torch = self._torch
        for index, item in enumerate(frames):
            fp = None
            if isinstance(item, tuple):
                if len(item) != 2 or not (item[1] is None or isinstance(item[1], FrameParams)):
                    raise ValueError(f"frame {index}: expected a frame or a (frame, FrameParams) pair")
                item, fp = item
            if isinstance(item, np.ndarray):
                if item.dtype != self._np_depth:
                    raise ValueError(f"frame {index}: dtype {item.dtype}, the stream's depth format takes {self._np_depth}")
                if item.ndim != 2:
                    raise ValueError(f"frame {index}: expected an (H, W) array, got shape {item.shape}")
                h, w = item.shape
                if w > 1 and item.strides[1] != item.itemsize:
                    raise ValueError(f"frame {index}: texels of a row are not contiguous (strides {item.strides})")
                location, stride = P.HOST, w              # staged packed, whatever the array's row stride
            elif isinstance(item, torch.Tensor):
                if item.device != self._device:
                    raise ValueError(f"frame {index}: a tensor on {item.device}; the stream takes tensors on {self._device} "
                                     "and host frames as NumPy arrays")
                if item.dtype != self._torch_depth:
                    raise ValueError(f"frame {index}: dtype {item.dtype}, the stream's depth format takes {self._torch_depth}")
                if item.dim() != 2:
                    raise ValueError(f"frame {index}: expected an (H, W) tensor, got shape {tuple(item.shape)}")
                h, w = item.shape
                if w > 1 and item.stride(1) != 1:
                    raise ValueError(f"frame {index}: texels of a row are not contiguous (stride(-1) = {item.stride(1)})")
                stride = item.stride(0) if h > 1 else w
                if stride < w:
                    raise ValueError(f"frame {index}: rows overlap (stride(-2) = {stride} < width {w})")
                location = P.DEVICE
            else:
                raise ValueError(f"frame {index}: expected a NumPy array or a torch tensor, got {type(item).__name__}")
            if not self._reserved and (w, h) != self.capacity:
                raise ValueError(f"frame {index}: {w} x {h} is not the stream's size {self.capacity[0]} x {self.capacity[1]}; "
                                 "construct the stream with max_size=(W, H) to take frames of changing sizes")
            store[index] = (item, fp)
            yield w, h, stride, fp is not None, location

    def _slots(self):
        """Pinned and device slots for host frames, allocated once, for `batch` frames of the capacity."""
        if self._depth_slots is None:
            torch = self._torch
            cw, ch = self.capacity
            self._depth_slots = _Slots(torch, P.DEPTH_SLOTS, self.batch * _aligned(cw * ch * self._np_depth.itemsize), self._device)
            self._result_slots = _Slots(torch, P.RESULT_SLOTS, self.batch * _aligned(cw * ch * self._np_ao.itemsize), self._device)
            self._upload, self._download = torch.cuda.Stream(self._device), torch.cuda.Stream(self._device)
        return self._depth_slots, self._result_slots

    # ---- the loop ----------------------------------------------------------------------
    def _run_generator(self, frames: Iterable) -> Iterator:
        torch, ao = self._torch, self.ao
        if self._active:
            raise RuntimeError("FrameStream.run: another run of this stream is still active")
        if not ao._ctx:
            raise RuntimeError("FrameStream.run: the stream is closed")
        compute = torch.cuda.current_stream(self._device)
        handle = compute.cuda_stream or _LEGACY_STREAM
        ao._sync_params()                      # pending property changes now: none can follow while the run is active
        store: dict = {}                       # frame index -> (frame, FrameParams | None), until its result has been yielded
        planner = P.Planner(self._describe(frames, store), self.batch, self.capacity, size=(ao.width, ao.height))
        live: dict = {}                        # step index -> what the ops of that step share
        run = _Run()
        self._active, ao._run = True, run
        fresh = carried = False                # the context holds an announcement / a ready set made from one
        stats = self._stats
        try:
            for op in planner:
                kind = type(op)
                if kind is P.Upload:
                    self._do_upload(planner.steps[op.step], op.slot, store, live)
                elif kind is P.WaitUploaded:
                    live[op.step]["uploaded"].synchronize()
                elif kind is P.Announce:
                    st = self._state(planner.steps[op.step], store, live)
                    ao.prefetch_device(st["depth"], st["params"], depth_pitch=st["pitch"], size=st["size"] if op.sized else None)
                    fresh = True
                    stats["announced"] += 1
                    stats["sized_announcements"] += op.sized
                elif kind is P.Execute:
                    step = planner.steps[op.step]
                    self._do_execute(step, self._state(step, store, live), compute, handle)
                    fresh, carried = False, fresh          # consumed the ready set, made the announcement the next one
                    stats["steps"] += 1
                    stats["frames"] += step.count
                elif kind is P.Resize:
                    ao.resize(op.w, op.h)
                    stats["resizes"] += 1
                elif kind is P.Download:
                    self._do_download(planner.steps[op.step], op.slot, live[op.step])
                else:
                    step = planner.steps[op.step]
                    results = self._results(step, live.pop(op.step))
                    for f in range(step.first, step.first + step.count):
                        del store[f]
                    for r in results:
                        run.frames_out += 1
                        yield r
        finally:
            self._active, ao._run = False, None
            if live and ao._ctx:
                # the run was abandoned, or a call failed, with steps in flight: let their work end before the frames and slots it
                # uses can go (the one place a run synchronises the compute stream)
                compute.synchronize()
                if self._upload is not None:
                    self._upload.synchronize()
                    self._download.synchronize()
            if (fresh or carried) and ao._ctx:
                ao._dirty = True               # a call that will not come was announced: meao_set_params withdraws it
                ao._sync_params()

    def _state(self, step: P.Step, store: dict, live: dict) -> dict:
        """What the calls of a step share: its pointers, pitch and parameter objects -- the announcement and the consuming call
        are given the same ones."""
        st = live.setdefault(step.index, {})
        if "depth" not in st:
            items = [store[f] for f in range(step.first, step.first + step.count)]
            st["size"] = step.size
            st["params"] = [fp for _, fp in items] if step.has_params else None
            if not step.host:
                st["inputs"] = [t for t, _ in items]
                st["depth"] = [t.data_ptr() for t in st["inputs"]]
                st["pitch"] = packed_pitch(step.stride * self._np_depth.itemsize, step.width, self._np_depth.itemsize)
        return st

    def _do_upload(self, step: P.Step, slot: int, store: dict, live: dict) -> None:
        torch = self._torch
        depth, _ = self._slots()
        st = self._state(step, store, live)
        w, h = step.size
        row, frame = w * self._np_depth.itemsize, _aligned(w * h * self._np_depth.itemsize)
        host, pin, dev = depth.host[slot], depth.pin[slot], depth.dev[slot]
        with torch.cuda.stream(self._upload):
            if depth.free_after[slot] is not None:       # the call that last read this slot, ordered on the device
                self._upload.wait_event(depth.free_after[slot])
            for i in range(step.count):                  # frame by frame: the copy of one runs while the next is staged
                lo, hi = i * frame, i * frame + h * row
                np.copyto(host[lo:hi].view(self._np_depth).reshape(h, w), store[step.first + i][0])
                dev[lo:hi].copy_(pin[lo:hi], non_blocking=True)
            st["uploaded"] = torch.cuda.Event()
            st["uploaded"].record(self._upload)
        base = depth.dev[slot].data_ptr()
        st["depth"], st["pitch"], st["depth_slot"] = [base + i * frame for i in range(step.count)], 0, slot

    def _do_execute(self, step: P.Step, st: dict, compute, handle: int) -> None:
        torch, ao = self._torch, self.ao
        w, h = step.size
        if step.host:
            depth, result = self._slots()
            frame = _aligned(w * h * self._np_ao.itemsize)
            base = result.dev[step.result_slot].data_ptr()
            out = [base + i * frame for i in range(step.count)]
            compute.wait_event(st["uploaded"])
        else:
            with torch.cuda.stream(compute):
                st["outputs"] = torch.empty((step.count, h, w), dtype=self._torch_ao, device=self._device)
            base, frame = st["outputs"].data_ptr(), w * h * self._np_ao.itemsize
            out = [base + i * frame for i in range(step.count)]
        ao.execute_device(st["depth"], out, stream=handle, params=st["params"], depth_pitch=st["pitch"])
        if step.host:
            st["executed"] = torch.cuda.Event()
            st["executed"].record(compute)
            depth.free_after[st["depth_slot"]] = st["executed"]

    def _do_download(self, step: P.Step, slot: int, st: dict) -> None:
        torch = self._torch
        _, result = self._slots()
        w, h = step.size
        used = (step.count - 1) * _aligned(w * h * self._np_ao.itemsize) + w * h * self._np_ao.itemsize
        with torch.cuda.stream(self._download):
            self._download.wait_event(st["executed"])
            result.pin[slot][:used].copy_(result.dev[slot][:used], non_blocking=True)
            st["downloaded"] = torch.cuda.Event()
            st["downloaded"].record(self._download)

    def _results(self, step: P.Step, st: dict) -> list:
        if not step.host:
            return list(st["outputs"].unbind(0))
        _, result = self._slots()
        w, h = step.size
        nbytes = w * h * self._np_ao.itemsize
        frame = _aligned(nbytes)
        st["downloaded"].synchronize()
        host = result.host[step.result_slot]
        return [host[i * frame:i * frame + nbytes].view(self._np_ao).reshape(h, w).copy() for i in range(step.count)]
