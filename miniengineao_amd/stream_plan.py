"""The schedule of a pipelined stream of frames, as data (miniengineao_amd.stream.FrameStream executes it).

Pure Python: this module imports neither torch nor the library, so the order of the calls -- the part of the pipelined loop that
include/meao.h states as rules -- can be checked without a GPU (tests/test_frame_stream_plan.py).

Frames are grouped in input order into STEPS of at most ``batch`` frames; one step is one execute call.  A step is uniform in size,
row stride, location (host or device) and presence of per-frame parameters: a frame that differs from the open step closes it
early (a mixed-size call has no announcement form and consumes a ready set unmatched, so none is ever planned).  A full step is
closed without looking at the next frame.

The ops of step i, in the order they are emitted (steady state):

    WaitUploaded(i+1)            host steps only: the announced buffers must be complete before the carrying call is submitted
    Announce(i+1, sized)         sized = step i+1 has another size than step i (meao_prefetch_batch_sized)
    Execute(i)                   consumes the announcement made for it, carries the pass of step i+1
    Resize(w, h)                 exactly when sized: the size of step i+1; keeps the sized announcement
    Download(i, slot)            host steps only; runs while Execute(i+1) does
    Yield(i-1)                   the host waits for Download(i-1) here, with Execute(i) already submitted
    Upload(i+2, slot)            host steps only; reads the input up to the end of step i+2

so between an announcement and the call that consumes it the context sees only the carrying call, that one resize and the next
announcement -- nothing that drops an announcement.  The last step announces nothing.  A host step's depth slot is read by
Execute(i-1) (the carried pass) and by Execute(i); Upload(i+2) goes into the slot that step i-1 held while Execute(i) may still
be running, which is what makes the depth slots three.  Its result slot is live from Execute(i) to Yield(i), and Yield(i-1)
follows Execute(i): two.

Look-ahead: when Yield(k) is emitted the planner has closed step k+2 and no later one.  It has read exactly the frames of the
steps up to k+2, and one frame more only where step k+2 was closed early by a frame that differs from it (that frame opens
step k+3; there is no other way to learn that a step which is not full has ended).

Errors: a frame outside the capacity, or a ValueError raised by the metadata iterator for a frame it cannot accept, ends the
input in front of that frame.  Every earlier step is still executed and yielded; the error is raised after the last Yield.
"""
from __future__ import annotations

from typing import Iterable, Iterator, List, NamedTuple, Optional, Tuple

HOST, DEVICE = "host", "device"
DEPTH_SLOTS, RESULT_SLOTS = 3, 2


class _Tagged:
    """Ops are tuples tagged by their class: Execute(0) is not Yield(0)."""
    __slots__ = ()

    def __eq__(self, other):
        return type(other) is type(self) and tuple.__eq__(self, other)

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((type(self).__name__,) + tuple(self))


class Upload(_Tagged, NamedTuple("Upload", [("step", int), ("slot", int)])):
    __slots__ = ()


class WaitUploaded(_Tagged, NamedTuple("WaitUploaded", [("step", int)])):
    __slots__ = ()


class Announce(_Tagged, NamedTuple("Announce", [("step", int), ("sized", bool)])):
    __slots__ = ()


class Execute(_Tagged, NamedTuple("Execute", [("step", int)])):
    __slots__ = ()


class Resize(_Tagged, NamedTuple("Resize", [("w", int), ("h", int)])):
    __slots__ = ()


class Download(_Tagged, NamedTuple("Download", [("step", int), ("slot", int)])):
    __slots__ = ()


class Yield(_Tagged, NamedTuple("Yield", [("step", int)])):
    __slots__ = ()


class Step(NamedTuple):
    """Frames first .. first + count - 1 of the input; stride in texels; depth_slot / result_slot: -1 for a device step."""
    index: int
    first: int
    count: int
    width: int
    height: int
    stride: int
    has_params: bool
    location: str
    depth_slot: int
    result_slot: int

    @property
    def size(self) -> Tuple[int, int]:
        return self.width, self.height

    @property
    def host(self) -> bool:
        return self.location == HOST


class PlanError(ValueError):
    """A frame the stream cannot take.  ``frame``: its index in the input; ``ops``: what plan() had emitted (plan() only)."""

    def __init__(self, frame: int, message: str):
        super().__init__(message)
        self.frame = frame
        self.ops: list = []


class Planner:
    """The incremental form: iterate it for the ops.  ``frames_meta`` yields (width, height, row_stride_texels, has_params,
    location) per frame and is consumed lazily (see the module docstring for how far ahead); ``steps`` holds the steps closed
    so far, ``frames_read`` the number of frames requested.  ``size``: the context's size before the first step, where a
    Resize has to bring it to the first step's; None = it is the first step's size."""

    def __init__(self, frames_meta: Iterable[tuple], batch: int, capacity: Tuple[int, int], size: Optional[Tuple[int, int]] = None):
        if batch < 1:
            raise ValueError("batch must be at least 1")
        self.steps: List[Step] = []
        self.frames_read = 0
        self._meta = iter(frames_meta)
        self._batch, self._capacity, self._size = int(batch), (int(capacity[0]), int(capacity[1])), size
        self._open: list = []                  # (frame index, meta) of the step being filled
        self._done = False
        self._error: Optional[ValueError] = None
        self._host_steps = 0

    def _append(self, frames: list) -> None:
        first, (w, h, stride, has_params, location) = frames[0]
        host = location == HOST
        self.steps.append(Step(len(self.steps), first, len(frames), w, h, stride, has_params, location,
                               self._host_steps % DEPTH_SLOTS if host else -1, self._host_steps % RESULT_SLOTS if host else -1))
        self._host_steps += host

    def _close_next(self) -> bool:
        """Reads frames until one more step is closed.  False: the input has ended and nothing was left."""
        while not self._done and len(self._open) < self._batch:
            index = self.frames_read
            try:
                meta = next(self._meta)
            except StopIteration:
                self._done = True
                break
            except ValueError as e:            # the frame is refused by whoever describes the frames
                self._done, self._error = True, e
                break
            self.frames_read += 1
            w, h, stride, has_params, location = meta
            meta = (int(w), int(h), int(stride), bool(has_params), location)
            if location not in (HOST, DEVICE):
                raise ValueError(f"frame {index}: location {location!r} is neither {HOST!r} nor {DEVICE!r}")
            if not (1 <= meta[0] <= self._capacity[0] and 1 <= meta[1] <= self._capacity[1]):
                self._done = True
                self._error = PlanError(index, f"frame {index}: {meta[0]} x {meta[1]} is outside the stream's capacity "
                                               f"{self._capacity[0]} x {self._capacity[1]} (max_size)")
                break
            if self._open and self._open[0][1] != meta:
                closed, self._open = self._open, [(index, meta)]
                self._append(closed)
                return True
            self._open.append((index, meta))
        if self._open:
            closed, self._open = self._open, []
            self._append(closed)
            return True
        return False

    def __iter__(self) -> Iterator[tuple]:
        steps = self.steps
        if self._close_next():
            if self._size is not None and tuple(self._size) != steps[0].size:
                yield Resize(*steps[0].size)
            if steps[0].host:
                yield Upload(0, steps[0].depth_slot)
            if self._close_next() and steps[1].host:
                yield Upload(1, steps[1].depth_slot)
        i = 0
        while i < len(steps):
            s = steps[i]
            nxt = steps[i + 1] if i + 1 < len(steps) else None
            sized = nxt is not None and nxt.size != s.size
            if nxt is not None:
                if nxt.host:
                    yield WaitUploaded(i + 1)
                yield Announce(i + 1, sized)
            yield Execute(i)
            if sized:
                yield Resize(*nxt.size)
            if s.host:
                yield Download(i, s.result_slot)
            if i >= 1:
                yield Yield(i - 1)
            if nxt is not None and self._close_next() and steps[i + 2].host:
                yield Upload(i + 2, steps[i + 2].depth_slot)
            i += 1
        if steps:
            yield Yield(len(steps) - 1)
        if self._error is not None:
            raise self._error


def plan(frames_meta: Iterable[tuple], batch: int, capacity: Tuple[int, int], size: Optional[Tuple[int, int]] = None) -> list:
    """The whole schedule of a finite input as a list of ops.  A frame outside the capacity raises PlanError, whose ``ops``
    holds the schedule of the frames in front of it."""
    ops: list = []
    try:
        for op in Planner(frames_meta, batch, capacity, size):
            ops.append(op)
    except PlanError as e:
        e.ops = ops
        raise
    return ops


def steps_of(frames_meta: Iterable[tuple], batch: int, capacity: Tuple[int, int]) -> List[Step]:
    """The steps plan() groups a finite, acceptable input into."""
    p = Planner(frames_meta, batch, capacity)
    for _ in p:
        pass
    return p.steps
