"""A model of the host-visible state of a meao context (and of a pool of them), and a generator of legal call sequences.

Written from include/meao.h and INTEGRATION.md alone: pure Python, no GPU, no ctypes, and nothing of the library's launch
planning.  The model predicts WHETHER things happen -- a call runs its own downsample pass or reuses a prefetched one, it carries an
announced pass, a waiting composite rides in its render launch or runs as plain launches -- never which tile shapes do it.
tests/test_call_sequences_gpu.py drives the real library and this model side by side; tests/test_call_model.py checks on the CPU that
the committed seeds reach the histories the GPU tests are meant to see; tools/fuzz_gpu.py --sequences draws fresh seeds.

Buffers, streams and parameter sets are abstract here: a buffer is an integer id, a stream 0 or 1, a parameter set a `Param` that
says what the model needs to know of a meao_params (the three Z-buffer inputs of the reuse key, and whether its tolerances keep a
call inside the exact-division range).  The driver maps them to tensors, hipStream_t and FrameParams.

What the header leaves to interpretation and this model fixes (DESIGN.md section 3 repeats them):
  * "a per-frame call" (the ring of eight, the composite that cannot ride) is a call that reads per-frame constants: one given
    params[], or one that carries an announcement made with params[].
  * "plain composite launches" are one launch per frame, as meao_composite is.
  * A HOST depth call is staged into context memory, so it never matches a ready set (another pointer); it still carries.
  * meao_reserve, when it succeeds, leaves nothing "as left by the last execute": the buffers moved, so meao_get_intermediate
    refuses until the next execute, as after a resize -- also when the reservation is the one the context had, or (0, 0) drops none.
  * The size is a component of the reuse key, and where it differs the pitch is not compared: a row stride of another width says
    nothing.  (Pitch option 3 gives two sizes one stride, so that the size is then the ONLY difference.)
  * What a resize keeps is from then on an ordinary announcement / ready set of the context's size: a second resize drops it, also
    one to the size the context has.  A resize to the current size is a resize like any other: it keeps nothing, since a sized
    announcement is by definition for another size.
  * A pool's announcement (announced_n) lives exactly as long as its members' shares: meao_pool_resize keeps or drops it whole.
"""
from __future__ import annotations

import dataclasses
import random
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

RING = 8                                           # meao.h: "a ring of 8 slots"
OK, ERR_INVALID_ARGUMENT = 0, -1
KEY_COMPONENTS = ("size", "pointer", "n", "stream", "pitch", "zb", "exact")
PITCH_EXTRA = (0, 8, 5)                            # pitch option -> texels beyond the row: packed, 4-texel vectors possible, scalar only
PITCH_FIXED = 408                                  # pitch option 3: this row stride whatever the width (a viewport of changing size in
#                                                    one allocation): a frame announced at one size and asked for at another then
#                                                    differs from the ready set in its size ALONE


def row_texels(option: int, width: int) -> int:
    """Row stride in texels of a surface of `width` under a pitch option."""
    return PITCH_FIXED if option == 3 else width + PITCH_EXTRA[option]


def f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


@dataclass(frozen=True)
class Param:
    """A meao_params as far as the model reads it.  tag: the driver's index into its palette of full parameter sets."""
    tag: int
    near: float
    far: float
    reversed_z: bool
    exact: bool = True          # tolerances inside the exact-division range (under RTZ storage)
    valid: bool = True          # meao_set_params would accept it

    def zb(self, linear: bool) -> tuple:
        if linear:              # "A prefetched downsample pass is reused when each frame's s matches": s = f32 nearest 1 / far_clip
            return (f32(1.0 / f32(self.far)),)
        return (f32(self.near), f32(self.far), bool(self.reversed_z))


@dataclass(frozen=True)
class Announcement:
    bufs: Tuple[int, ...]
    pitch: int                                  # row stride in texels (packed = width)
    params: Optional[Tuple[Param, ...]]         # None: the context's parameters at the time of the carrying call
    sized: bool = False                         # meao_prefetch_batch_sized for another size than the context's
    size: Tuple[int, int] = (0, 0)              # of the announced frames


@dataclass(frozen=True)
class ReadySet:
    bufs: Tuple[int, ...]
    stream: int
    pitch: int
    zb: Tuple[tuple, ...]
    exact: bool                                 # the carrying call divided exactly (it stamped the hostile flags)
    sized: bool = False                         # it came from a sized announcement: a resize to its size keeps it
    size: Tuple[int, int] = (0, 0)              # of the frames its levels were built from
    kept: bool = False                          # a resize kept it


@dataclass(frozen=True)
class Composite:
    mode: int
    ao: Tuple[int, ...]
    color: Tuple[int, ...]
    stream: int                                 # of the execute before the enqueue: where a flush without a stream runs it


@dataclass(frozen=True)
class LastCall:
    n: int
    params: Tuple[Param, ...]                   # per frame, as the call used them
    bufs: Tuple[int, ...]
    outs: Tuple[int, ...]
    depth_pitch: int
    out_pitch: int
    depth_host: bool
    out_host: bool
    stream: int
    exact: bool
    reused: bool
    had_ready: bool = False                     # a ready set existed when the call was made (it is gone after it)
    shared: bool = True                         # the call used the context's parameters (no params[])


@dataclass
class Op:
    """One host action.  kind: prefetch | execute | set_params | resize | reserve | comp_enqueue | comp_flush | debug_set | refill |
    invalid.  `size` is the new size of a resize, the reservation of a reserve ((0, 0) drops it), the announced size of a prefetch
    (None: the context's, the ordinary announcement) and the size of the frames a refill lays out (None: the context's)."""
    kind: str
    bufs: Tuple[int, ...] = ()
    outs: Tuple[int, ...] = ()
    params: Optional[Tuple[Param, ...]] = None
    pitch: int = 0                              # pitch OPTION of the depth surfaces (index into PITCH_EXTRA)
    out_pitch: int = 0
    depth_host: bool = False
    out_host: bool = False
    stream: int = 0
    param: Optional[Param] = None               # set_params
    size: Optional[Tuple[int, int]] = None      # resize, reserve, prefetch, refill (see above)
    mode: int = 0                               # comp_enqueue
    colors: Tuple[int, ...] = ()
    key: int = 0                                # debug_set
    value: int = 0
    contents: Tuple[tuple, ...] = ()            # refill: one content key per buffer of bufs
    what: str = ""                              # invalid: bad_pitch | n_zero | n_over | bad_params | null_pointer | SIZED_INVALID
    on: str = ""                                # invalid: execute | prefetch | reserve | resize
    read_debug: bool = False                    # stepped mode: compare debug buffers after this execute


@dataclass
class Expect:
    status: int = OK
    launched: bool = False                      # the call enqueued kernels
    own_pass: bool = False                      # execute: its own downsample pass runs
    reused: bool = False
    refused: Tuple[str, ...] = ()               # a ready set existed and was refused: the key components that differ
    carried: Optional[Announcement] = None      # the announced pass this call carries
    per_frame: bool = False                     # takes a slot of the ring of eight
    comp_carried: int = 0                       # frames of a composite riding in this call's render launch
    comp_plain: int = 0                         # frames of a composite run as plain launches by this operation
    comp_ran: Optional[Composite] = None
    comp_pending: int = 0                       # frames waiting after the operation
    reallocated: bool = False                   # first announcement of a context created without cfg.pipelined
    last_valid: bool = False                    # meao_get_intermediate answers after the operation
    exact: bool = False
    events: List[str] = field(default_factory=list)   # coverage classes (tests/test_call_model.py)


# the invalid calls of dynamic resolution (Op.what); Op.on says which call makes them
SIZED_INVALID = ("sized_outside_reservation", "sized_without_reservation", "sized_bad_pitch", "reserve_below_current",
                 "pool_resize_uncovered")


class ContextModel:
    def __init__(self, width, height, max_batch, param: Param, *, linear=False, rtz=True, pipelined=True, exhaustive=False,
                 cap=(0, 0)):
        self.width, self.height, self.max_batch = width, height, max_batch
        self.param, self.linear, self.rtz, self.exhaustive = param, linear, rtz, exhaustive
        self.two_sets = pipelined
        self.cap: Tuple[int, int] = tuple(cap)      # the reservation (meao_get_capacity); (0, 0): none
        self.dropped: Optional[ReadySet] = None     # coverage only: the ready set a resize dropped since the last call
        self.ann: Optional[Announcement] = None
        self.ready: Optional[ReadySet] = None
        self.comp: Optional[Composite] = None
        self.ring = 0
        self.last: Optional[LastCall] = None
        self.last_intact = False                    # the depth frames of the last call have not been refilled since
        self.contents: Dict[int, tuple] = {}        # the host's side of the contract: what each depth buffer holds
        self.fresh: set = set()                     # buffers refilled since a call last read them
        self.totals = {"own": 0, "carried": 0, "reused": 0, "comp_carried_launches": 0, "comp_plain_launches": 0, "per_frame": 0, "carried_more": 0,
                       "carried_sized": 0, "kept_by_resize": 0}

    # ---- helpers
    def pitch_texels(self, option: int, width=None) -> int:
        return row_texels(option, self.width if width is None else width)

    def within(self, w, h) -> bool:
        """'a size inside the reservation (both dimensions)'; without a reservation nothing is."""
        return self.cap != (0, 0) and w <= self.cap[0] and h <= self.cap[1]

    def _exact(self, params) -> bool:
        return self.rtz and all(p.exact for p in params)

    def _expect(self, **kw) -> Expect:
        e = Expect(**kw)
        e.comp_pending = len(self.comp.ao) if self.comp else 0
        e.last_valid = self.last is not None
        return e

    def _run_comp_plain(self, e: Expect, why: str) -> None:
        e.comp_ran, e.comp_plain = self.comp, len(self.comp.ao)
        self.totals["comp_plain_launches"] += e.comp_plain
        e.events.append("comp_flushed_by_" + why)
        self.comp = None

    def referenced(self, buf: int) -> bool:
        """The host may not refill a depth buffer an announcement or a ready set refers to."""
        return (self.ann is not None and buf in self.ann.bufs) or (self.ready is not None and buf in self.ready.bufs)

    def ao_waiting(self, buf: int) -> bool:
        return self.comp is not None and buf in self.comp.ao

    # ---- operations
    def refill(self, bufs, contents, pitch=0) -> Expect:
        for b, c in zip(bufs, contents):
            assert not self.referenced(b), "illegal sequence: refill of an announced / ready buffer"
            self.contents[b] = (c, pitch)
            self.fresh.add(b)
            self.touched(b)
        return self._expect()

    def touched(self, buf) -> None:
        if self.last is not None and buf in self.last.bufs:
            self.last_intact = False                # debug id 1 is built from the depth frame the last execute was given

    def readable(self) -> bool:
        """Everything "as left by the last execute" can be read back and compared: there was one, and its frames are unchanged."""
        return self.last is not None and self.last_intact

    def invalid(self, op: Op) -> Expect:
        """The documented status, nothing launched, state unchanged."""
        status = ERR_INVALID_ARGUMENT
        e = self._expect(status=status)
        if op.what in SIZED_INVALID:                 # the generator's claim that the call is invalid, held to the rule it names
            cur = (self.width, self.height)
            if op.what == "sized_without_reservation":
                assert self.cap == (0, 0) and tuple(op.size) != cur, op
            elif op.what == "sized_outside_reservation":
                assert self.cap != (0, 0) and not self.within(*op.size), op
            elif op.what == "sized_bad_pitch":       # the pitch is the only thing wrong with it
                assert self.within(*op.size) and tuple(op.size) != cur, op
            elif op.what == "reserve_below_current":
                assert self.reserve(*op.size).status == ERR_INVALID_ARGUMENT, op
            elif op.what == "pool_resize_uncovered":
                assert not self.within(*op.size), op
            e.events.append("invalid_" + op.what)
            if self.ann is not None and self.ann.sized:
                e.events.append("invalid_while_sized_announced")
        if self.ann is not None:
            e.events.append("invalid_while_announced")
        if self.comp is not None:
            e.events.append("invalid_while_composite")
        if self.readable():
            e.events.append("debug_read_after_invalid")
        return e

    def prefetch(self, bufs, params=None, pitch=0, size=None, pitch_texels=None) -> Expect:
        """size: meao_prefetch_batch_sized.  pitch_texels: a row stride given outright instead of a pitch option (the model's own
        tests; the sequences name their one illegal stride by Op.what)."""
        cur = (self.width, self.height)
        sized = size is not None and tuple(size) != cur      # "with width x height equal to the current size the call IS ..._pitched"
        w, h = tuple(size) if sized else cur
        if sized and not self.within(w, h):
            return self._expect(status=ERR_INVALID_ARGUMENT)
        rows = self.pitch_texels(pitch, w) if pitch_texels is None else pitch_texels
        if rows < w:                                  # "depth_pitch is validated against the ANNOUNCED size"
            return self._expect(status=ERR_INVALID_ARGUMENT)
        e = Expect()
        if not self.two_sets:
            self.two_sets = True                 # re-allocates: geometry unchanged, everything "as left by the last execute" gone
            e.reallocated = True                 # (and the reservation unchanged: self.cap is not touched)
            e.events.append("first_announcement_reallocates")
            if sized:
                e.events.append("sized_first_announcement_reallocates")
            self.last = None
            self.ready = None
        if self.ann is not None:
            e.events.append("announcement_replaced")
        if sized:
            e.events.append("sized_announcement")
            if params is not None:
                e.events.append("sized_per_frame")
            if rows != w:
                e.events.append("sized_pitched")
            if rows < self.width:
                e.events.append("sized_pitch_below_current_width")
            if self.comp is not None:
                e.events.append("sized_announced_while_composite")
        self.ann = Announcement(tuple(bufs), rows, None if params is None else tuple(params), sized, (w, h))
        e.comp_pending = len(self.comp.ao) if self.comp else 0
        e.last_valid = self.last is not None
        return e

    def execute(self, bufs, outs, params=None, pitch=0, out_pitch=0, depth_host=False, out_host=False, stream=0) -> Expect:
        n = len(bufs)
        assert 1 <= n <= self.max_batch and len(outs) == n
        prm = tuple(params) if params is not None else (self.param,) * n
        exact = self._exact(prm)
        depth_pitch = self.width if depth_host else self.pitch_texels(pitch)      # HOST frames are staged packed
        assert depth_pitch >= self.width, "illegal sequence: a row stride below the width"
        e = Expect(launched=True, exact=exact)
        for b in bufs:
            if b in self.fresh:
                e.events.append("refilled_before_call")
                break

        # own pass iff the ready set does not match in EVERY key component; the ready set is gone either way
        def differs(r):
            m = min(n, len(r.bufs))
            diff = []
            other_size = r.size != (self.width, self.height)
            if other_size:                          # "the consuming execute matches on the size as well"
                diff.append("size")
            if depth_host or tuple(bufs[:m]) != r.bufs[:m]:
                diff.append("pointer")
            if n != len(r.bufs):
                diff.append("n")
            if stream != r.stream:
                diff.append("stream")
            if depth_pitch != r.pitch and not other_size:      # (a row stride of another width says nothing: "size" stands for it)
                diff.append("pitch")
            if tuple(p.zb(self.linear) for p in prm[:m]) != r.zb[:m]:
                diff.append("zb")
            if exact and not r.exact:
                diff.append("exact")
            return diff, other_size

        r = self.ready
        if r is None and self.dropped is not None and not differs(self.dropped)[0]:
            e.events.append("asked_for_what_a_resize_dropped")      # exactly what a ready set that outlived the resize would serve
        self.dropped = None
        if r is not None:
            diff, other_size = differs(r)
            e.refused = tuple(diff)
            e.reused = not diff
            if other_size and depth_pitch == r.pitch:
                e.events.append("other_size_same_stride")
            if e.reused:
                e.events.append("reuse")
                if r.kept:
                    e.events.append("reuse_of_kept_sized_ready" if self.ann is None else "reuse_of_kept_sized_ready_while_carrying")
            elif len(diff) == 1:
                e.events.append("refused_" + diff[0])
        elif (self.last is not None and self.last.had_ready and not depth_host and not self.last.depth_host
              and (tuple(bufs), depth_pitch, stream) == (self.last.bufs, self.last.depth_pitch, self.last.stream)):
            e.events.append("asked_again_after_ready_gone")     # what a ready set that outlived its one call would serve
        e.own_pass = not e.reused
        self.ready = None

        # the announced pass is carried by this call and becomes the ready set
        a = self.ann
        e.per_frame = params is not None or (a is not None and a.params is not None)
        if a is not None:
            e.carried = a
            aprm = a.params if a.params is not None else (self.param,) * len(a.bufs)
            # (an announcement that is not sized is for the context's size, whatever that was when it was made: no resize keeps it)
            self.ready = ReadySet(a.bufs, stream, a.pitch, tuple(p.zb(self.linear) for p in aprm), exact, a.sized,
                                  a.size if a.sized else (self.width, self.height))
            self.ann = None
            if a.sized:
                self.totals["carried_sized"] += 1
                e.events.append("sized_carried")
            if len(a.bufs) > n:
                self.totals["carried_more"] += 1
                e.events.append("announced_more_than_carrier")
                if a.sized:
                    e.events.append("sized_announced_more_than_carrier")
            elif len(a.bufs) < n:
                e.events.append("announced_fewer_than_carrier")
        if e.per_frame:
            self.ring = (self.ring + 1) % RING
            self.totals["per_frame"] += 1

        # a waiting composite rides in this call's render launch, or runs first as plain launches
        if self.comp is not None:
            if e.per_frame or self.exhaustive:
                self._run_comp_plain(e, "per_frame_call")
            else:
                e.comp_ran, e.comp_carried = self.comp, len(self.comp.ao)
                self.totals["comp_carried_launches"] += 1
                e.events.append("comp_carried")
                self.comp = None

        for b in bufs:
            self.fresh.discard(b)
        self.last = LastCall(n, prm, tuple(bufs), tuple(outs), depth_pitch, self.width if out_host else self.pitch_texels(out_pitch),
                             depth_host, out_host, stream, exact, e.reused, r is not None, params is None)
        self.last_intact = True
        self.totals["own"] += e.own_pass
        self.totals["reused"] += e.reused
        self.totals["carried"] += e.carried is not None
        e.last_valid = True
        return e

    def set_params(self, param: Param) -> Expect:
        e = Expect()
        if self.ann is not None:
            e.events.append("announcement_dropped_by_set_params")
        if self.ready is not None:
            e.events.append("ready_dropped_by_set_params")
        if self.readable() and self.last.shared and param != self.param:
            e.events.append("debug_read_after_set_params")     # the last call's parameters are no longer the context's
        self.param, self.ann, self.ready, self.dropped = param, None, None, None
        e.comp_pending = len(self.comp.ao) if self.comp else 0
        e.last_valid = self.last is not None
        return e

    def resize(self, width, height) -> Expect:
        e = Expect()
        if self.comp is not None:
            self._run_comp_plain(e, "resize")       # at the old size, on the stream that produced its AO
        inside = self.within(width, height)
        if (width, height) == (self.width, self.height) and (self.ann is not None or self.ready is not None):
            e.events.append("resize_to_current_size")          # a resize like any other: nothing can have been made for it
        keep = lambda x: inside and x is not None and x.sized and x.size == (width, height)       # noqa: E731
        for what, x in (("announcement", self.ann), ("ready", self.ready)):
            if x is None:
                continue
            if keep(x):
                e.events.append("sized_%s_kept_by_resize" % what)
                self.totals["kept_by_resize"] += 1
                if e.comp_plain:
                    e.events.append("comp_flushed_and_sized_kept")
                continue
            e.events.append(what + "_dropped_by_resize")
            if inside:
                e.events.append(("sized_%s_dropped_other_size" if x.sized else "unsized_%s_dropped_by_resize_inside") % what)
                if not x.sized:
                    e.events.append("unsized_dropped_by_resize_inside")
            elif x.sized:
                e.events.append("sized_dropped_by_resize_outside")
        if self.ready is not None and not keep(self.ready) and self.dropped is None:
            self.dropped = self.ready
        # a kept one is from now on an ordinary one for the context's size
        self.ann = dataclasses.replace(self.ann, sized=False) if keep(self.ann) else None
        self.ready = dataclasses.replace(self.ready, sized=False, kept=True) if keep(self.ready) else None
        if self.cap != (0, 0) and not inside:       # "the reservation grows to the component-wise maximum"
            self.cap = (max(self.cap[0], width), max(self.cap[1], height))
            e.events.append("resize_grows_reservation")
        self.width, self.height = width, height
        self.last = None
        e.comp_pending = 0
        return e

    def reserve(self, width, height) -> Expect:
        """meao_reserve.  (0, 0) drops the reservation; anything else must cover the current size."""
        drop = (width, height) == (0, 0)
        if not drop and (width < self.width or height < self.height):
            return self._expect(status=ERR_INVALID_ARGUMENT)
        e = Expect()
        if self.ann is not None:
            e.events.append("reserve_drops_announcement")
        if self.ready is not None:
            e.events.append("reserve_drops_ready")
        if self.comp is not None:
            e.events.append("reserve_keeps_composite")
        if drop and self.cap != (0, 0):
            e.events.append("reservation_dropped")
            if self.ready is not None and self.ready.sized:
                e.events.append("reservation_dropped_with_sized_ready")
        self.cap = (width, height)
        self.ann = self.ready = self.last = self.dropped = None     # the buffers moved: nothing "as left by the last execute" is left
        e.comp_pending = len(self.comp.ao) if self.comp else 0
        return e

    def comp_enqueue(self, mode, ao, colors) -> Expect:
        e = Expect()
        if self.comp is not None:
            self._run_comp_plain(e, "second_enqueue")
        self.comp = Composite(mode, tuple(ao), tuple(colors), self.last.stream if self.last else 0)
        e.comp_pending = len(ao)
        e.last_valid = self.last is not None
        return e

    def comp_flush(self) -> Expect:
        e = Expect()
        if self.comp is not None:
            self._run_comp_plain(e, "comp_flush")
        e.last_valid = self.last is not None
        return e

    def debug_set(self, key, value) -> Expect:
        e = self._expect()                          # a launch-structure key: no change of any result
        if self.readable():
            e.events.append("debug_read_after_debug_set")
        return e

    def drop_announcement(self, ready_too: bool) -> None:
        """Pool members only: a pool call that deals this member no frame (see PoolModel)."""
        self.ann = None
        if ready_too:
            self.ready = None

    def apply(self, op: Op) -> Expect:
        k = op.kind
        if k == "refill":
            return self.refill(op.bufs, op.contents, op.pitch)
        if k == "prefetch":
            e = self.prefetch(op.bufs, op.params, op.pitch, op.size)
            assert e.status == OK, ("illegal sequence: an announcement the library refuses", op)
            return e
        if k == "execute":
            return self.execute(op.bufs, op.outs, op.params, op.pitch, op.out_pitch, op.depth_host, op.out_host, op.stream)
        if k == "set_params":
            return self.set_params(op.param)
        if k == "resize":
            return self.resize(*op.size)
        if k == "reserve":
            e = self.reserve(*op.size)
            assert e.status == OK, ("illegal sequence: a reservation the library refuses", op)
            return e
        if k == "comp_enqueue":
            return self.comp_enqueue(op.mode, op.bufs, op.colors)
        if k == "comp_flush":
            return self.comp_flush()
        if k == "debug_set":
            return self.debug_set(op.key, op.value)
        if k == "invalid":
            return self.invalid(op)
        raise ValueError(k)


class PoolModel:
    """G context models plus the dealing rule (frame f -> member f mod G), at pool level: an announcement is for the call after next
    OF THE POOL.  A member that a pool execute deals no frame has been passed by that call: what it holds -- an announcement,
    a ready set -- was for a call that is over, and is dropped.  A pool announcement replaces the one before it in every member."""

    def __init__(self, G, width, height, max_batch, param, **kw):
        self.G, self.max_batch = G, max_batch
        self.members = [ContextModel(width, height, max_batch, param, **kw) for _ in range(G)]
        self.contents: Dict[int, tuple] = {}
        self.fresh: set = set()
        self.announced_n: Optional[int] = None       # frames of the pool announcement that waits

    width = property(lambda s: s.members[0].width)
    height = property(lambda s: s.members[0].height)
    param = property(lambda s: s.members[0].param)

    def share(self, m, seq):
        return tuple(seq[m::self.G])

    def referenced(self, buf):
        return any(c.referenced(buf) for c in self.members)

    def ao_waiting(self, buf):
        return any(c.ao_waiting(buf) for c in self.members)

    def _deal(self, op: Op, idle=None) -> List[Optional[Expect]]:
        out = []
        n = len(op.bufs)
        for m, c in enumerate(self.members):
            if m >= n:
                if idle:
                    idle(c)
                out.append(None)
                continue
            sub = dataclasses.replace(op, bufs=self.share(m, op.bufs), outs=self.share(m, op.outs), colors=self.share(m, op.colors),
                                      params=None if op.params is None else self.share(m, op.params))
            out.append(c.apply(sub))
        return out

    def apply(self, op: Op) -> List[Optional[Expect]]:
        """One Expect per member; None for a member the call deals no frame (it launches nothing).  The coverage classes of the
        pool itself go to the first Expect's events."""
        k = op.kind
        if k == "refill":
            for b, c in zip(op.bufs, op.contents):
                assert not self.referenced(b), "illegal sequence: refill of an announced / ready buffer"
                self.contents[b] = (c, op.pitch)
                self.fresh.add(b)
                for m in self.members:
                    m.touched(b)
            return [c._expect() for c in self.members]
        if k == "execute":
            n = len(op.bufs)
            idle_sized = [c for c in self.members[n:] if (c.ann is not None and c.ann.sized) or (c.ready is not None and c.ready.sized)]
            out = self._deal(op, lambda c: c.drop_announcement(True))
            ev = out[0].events
            if idle_sized:
                ev.append("pool_idle_member_drops_sized")
            if any(b in self.fresh for b in op.bufs):
                ev.append("refilled_before_call")
            self.fresh.difference_update(op.bufs)
            if n < self.G:
                ev.append("pool_n_below_members")
            if n % self.G:
                ev.append("pool_n_not_multiple")
            if self.announced_n is not None and self.announced_n != n:
                ev.append("pool_n_differs_from_announced")
            self.announced_n = None
            return out
        if k == "prefetch":
            self.announced_n = len(op.bufs)
            return self._deal(op, lambda c: c.drop_announcement(False))
        if k == "comp_enqueue":
            return self._deal(op)
        if k == "invalid":
            out = [c.invalid(op) for c in self.members]
            for e in out[1:]:
                e.events = [x for x in e.events if x not in out[0].events]      # a coverage class counts once per pool call
            return out
        if k == "set_params" or k == "reserve":          # (a reservation covers every member's size or none's: they are one size)
            self.announced_n = None
        if k == "resize":
            # "for sizes that EVERY member's reservation covers; anything else is MEAO_ERR_INVALID_ARGUMENT, checked for every
            # member before any member is touched"
            assert all(c.within(*op.size) for c in self.members), ("illegal sequence: a pool resize the library refuses", op)
            out = [c.apply(op) for c in self.members]
            if not any(c.ann is not None for c in self.members):
                self.announced_n = None                   # the pool's announcement lives exactly as long as its members' shares
            for e in out[1:]:
                e.events = [x for x in e.events if x not in out[0].events]
            return out
        return [c.apply(op) for c in self.members]      # set_params, reserve, comp_flush: every member


# ---- the generator -------------------------------------------------------------------------------------------------------------

@dataclass
class Profile:
    """Weights per operation and the shape of a sequence."""
    length: int = 40                   # operations, the refills of depth buffers not counted
    max_batch: int = 4
    sizes: Tuple[Tuple[int, int], ...] = ((384, 256), (380, 250))
    n_depth: int = 10                  # depth buffers
    n_out: int = 10                    # AO buffers (stepped mode; the free-running mode gives every call its own)
    n_color: int = 8
    free_running: bool = False         # DEVICE / DEVICE only, no resize, no debug reads: nothing that synchronises
    pool: int = 0                      # members (0: one context)
    w_execute: float = 10
    w_prefetch: float = 6
    w_set_params: float = 1.6
    w_resize: float = 1.6
    w_comp_enqueue: float = 2.5
    w_comp_flush: float = 1.0
    w_debug_set: float = 0.5
    w_invalid: float = 1.5
    p_honour: float = 0.5             # an execute after a carried announcement passes exactly what was announced ...
    p_vary_one: float = 0.4           # ... or differs from it in ONE key component; else it is unrelated
    p_per_frame: float = 0.45
    p_pitched: float = 0.25
    p_host: float = 0.12
    p_refill: float = 0.7              # a legal buffer about to be passed gets new contents under its pointer
    p_hostile: float = 0.25
    p_other_stream: float = 0.12
    p_follow_up: float = 0.55
    p_comp_ended_early: float = 0.45
    p_ann_disturbed: float = 0.2       # an announcement is followed by an invalid call or a resize
    p_again: float = 0.2
    p_set_params_after: float = 0.1    # a shared call is followed by other parameters: debug reads must still show the call's
    p_inexact_carrier: float = 0.3     # a carrying call gets a parameter set outside the exact-division range
    # dynamic resolution; the defaults draw nothing of it (and no random number for it: the older sequences stay as they are)
    reserve: Optional[Tuple[int, int]] = None    # the reservation: the first operation of a stepped sequence, the state a
    #                                              free-running one starts in (meao_reserve synchronises)
    w_reserve: float = 0.0             # meao_reserve in mid-sequence: the same again, larger, (0, 0), or one below the current size
    p_sized: float = 0.0               # share of announcements made for another size inside the reservation
    p_sized_then_resize: float = 0.0   # a sized announcement is followed by execute and a resize to its size (the header's frame
    #                                    loop), or by that resize at once
    outside_sizes: Tuple[Tuple[int, int], ...] = ()   # sizes no reservation of the sequence covers at first: stepped resizes go there

N_CONTENTS = 12                        # content keys are ("synth" | "hostile" | "hostile_level", seed < N_CONTENTS)
DEBUG_KEYS = ((0, (0, 1)), (1, (0, 1024)), (2, (0, 256)), (3, (0, 2048)), (4, (0, 640)), (5, (0, 1, 4096)))   # meao_debug_key -> values


def initial_cap(profile: Profile) -> Tuple[int, int]:
    """The reservation a sequence of this profile starts under: a free-running one is reserved before its first operation."""
    return tuple(profile.reserve) if profile.reserve and profile.free_running else (0, 0)


def generate(seed: int, profile: Profile, palette: List[Param], start_param: Param, *, linear=False, rtz=True, pipelined=True):
    """A legal sequence of Ops from a seed.  palette: the parameter sets per-frame calls and set_params draw from (an invalid one,
    if present, is used by invalid calls only).  The generator keeps a model of its own to stay inside the contract a host must
    keep: a depth buffer is refilled only when no announcement or ready set refers to it, an AO buffer whose composite waits is not
    written.  (Ordering across a change of stream, and "no enqueued work reads it", are the driver's: it orders the streams with an
    event wait at every change and refills in stream order.)  Returns the Ops; replay() runs them through a fresh model."""
    rng = random.Random(seed)
    P = profile
    G = P.pool
    valid = [p for p in palette if p.valid]
    inexact = [p for p in valid if not p.exact]
    bad = [p for p in palette if not p.valid]
    cap = P.max_batch * (G or 1)
    w, h = P.sizes[0]
    kw = dict(linear=linear, rtz=rtz, pipelined=pipelined, cap=initial_cap(P))
    model = PoolModel(G, w, h, P.max_batch, start_param, **kw) if G else ContextModel(w, h, P.max_batch, start_param, **kw)
    one = model.members[0] if G else model         # the members of a pool are one size and hold one reservation
    ops: List[Op] = []
    st = {"stream": 0, "next_out": 0, "promised": None, "announced": None, "last_exec": None, "flip": False, "loop": None,
          "uncovered": False}
    laid: Dict[int, tuple] = {}                    # depth buffer -> (size, pitch option) of the frame it holds

    def emit(op):
        ops.append(op)
        return model.apply(op)

    def legal_depth(k, avoid=()):
        free = [b for b in range(P.n_depth) if b not in avoid]
        rng.shuffle(free)
        return tuple(free[:k])

    def cur_size():
        return (model.width, model.height)

    def inside_sizes(other_than=None):
        return [s for s in P.sizes if s != other_than and one.within(*s)]

    def draw_outs(k):
        if P.free_running:
            st["next_out"] += k
            return tuple(range(st["next_out"] - k, st["next_out"]))
        free = [b for b in range(P.n_out) if not model.ao_waiting(b)]
        rng.shuffle(free)
        return tuple(free[:k])

    def draw_params(k):
        return tuple(rng.choice(valid) for _ in range(k))

    def content():
        r = rng.random()
        kind = "hostile_level" if r < P.p_hostile * 0.6 else "hostile" if r < P.p_hostile else "synth"
        return (kind, rng.randrange(N_CONTENTS))

    def maybe_refill(bufs, pitch, size=None):
        """size: the frames are announced at that size, and a buffer that does not hold a frame of it under this pitch gets one."""
        sel = tuple(b for b in bufs if not model.referenced(b) and
                    (b not in model.contents or (size is not None and laid.get(b) != (size, pitch)) or rng.random() < P.p_refill))
        for b in sel:
            laid[b] = (size or cur_size(), pitch)
        if sel:
            emit(Op("refill", bufs=sel, contents=tuple(content() for _ in sel), pitch=pitch, size=size))   # laid out for the call it is for

    def pitch_option():
        return rng.choice((1, 2)) if rng.random() < P.p_pitched else 0

    def sized_depth(k, size, pitch):
        """Buffers that hold a frame of `size` under `pitch`, or may be given one now (the free-running pool fills a buffer once)."""
        once = bool(G) and P.free_running
        ok = [b for b in range(P.n_depth) if laid.get(b) == (size, pitch) or
              (not model.referenced(b) and not (once and b in model.contents))]
        rng.shuffle(ok)
        return tuple(ok[:k])

    def do_sized_prefetch(k):
        """meao_prefetch_batch_sized for another size inside the reservation; False: there is none (or no buffer for it)."""
        sizes = inside_sizes(other_than=cur_size())
        if not sizes:
            if one.cap == (0, 0):
                if P.w_reserve and rng.random() < 0.5:
                    do_reserve()
                else:
                    do_invalid("sized_without_reservation")
            return False
        size, pitch = rng.choice(sizes), pitch_option()
        if rng.random() < 0.3 and max(size[0], model.width) <= PITCH_FIXED:
            pitch = 3                                # one stride for both sizes
        bufs = sized_depth(k, size, pitch)
        if not bufs:
            return False
        maybe_refill(bufs, pitch, size)
        prm = draw_params(len(bufs)) if rng.random() < P.p_per_frame else None
        op = Op("prefetch", bufs=bufs, params=prm, pitch=pitch, size=size)
        emit(op)
        st["announced"] = op
        r = rng.random()
        if r < P.p_sized_then_resize:
            if rng.random() < 0.35:
                do_resize(to=size)                   # at once: the announcement itself is kept, and carried at its own size
            else:
                if rng.random() < 0.3:
                    do_invalid()                     # an invalid call in between changes nothing
                st["loop"] = size                    # the header's frame loop: execute at the old size, then the resize
        elif r < P.p_sized_then_resize + P.p_ann_disturbed:
            rng.choice((do_invalid, do_set_params, do_resize) + ((do_reserve,) if P.w_reserve else ()))()
        return True

    def do_prefetch():
        k = rng.randint(1, cap)
        if P.p_sized and rng.random() < P.p_sized and do_sized_prefetch(k):
            return
        bufs = legal_depth(k)
        pitch = pitch_option()
        maybe_refill(bufs, pitch)
        prm = draw_params(k) if rng.random() < P.p_per_frame else None
        op = Op("prefetch", bufs=bufs, params=prm, pitch=pitch)
        emit(op)
        st["announced"] = op
        if rng.random() < P.p_ann_disturbed:
            if not G and not P.free_running and rng.random() < 0.5:
                do_resize()
            else:
                do_invalid()

    def vary_one(bufs, prm, pitch, stream):
        """What was announced, changed in one component of the reuse key."""
        which = rng.choice(("pointer", "n", "n", "stream", "pitch", "zb", "zb"))
        if which == "pointer":
            i = rng.randrange(len(bufs))
            bufs = bufs[:i] + legal_depth(1, avoid=bufs) + bufs[i + 1:]
        elif which == "n":
            if len(bufs) > 1 and (len(bufs) == cap or rng.random() < 0.5):
                bufs, prm = bufs[:-1], None if prm is None else prm[:-1]
            elif len(bufs) < cap:
                bufs = bufs + legal_depth(1, avoid=bufs)
                prm = None if prm is None else prm + (prm[-1],)
        elif which == "stream" and not G:
            stream = 1 - stream
        elif which == "pitch":
            pitch = (pitch + rng.choice((1, 2))) % 3
        elif which == "zb":
            base = prm if prm is not None else (model.param,) * len(bufs)
            i = rng.randrange(len(base))
            same_rest = [p for p in valid if p.zb(linear) != base[i].zb(linear) and p.exact == base[i].exact]
            if same_rest:
                prm = base[:i] + (rng.choice(same_rest),) + base[i + 1:]
        return bufs, prm, pitch, stream

    def do_execute():
        stream = st["stream"]
        host_d = host_o = False
        promised = st["promised"]
        r = rng.random()
        if st.pop("honour", False):
            r = 0.0
        if promised is not None and r < P.p_honour + P.p_vary_one:
            bufs, prm, pitch = promised.bufs, promised.params, promised.pitch
            if pitch == 3 and model.width > PITCH_FIXED:
                pitch = 0
            if r >= P.p_honour:
                bufs, prm, pitch, stream = vary_one(bufs, prm, pitch, stream)
        else:
            if not G and rng.random() < P.p_other_stream:
                stream = 1 - stream
            if not P.free_running and not G and rng.random() < P.p_host:
                host_d, host_o = rng.choice(((True, True), (True, False), (False, True)))
            k = rng.randint(1, cap)
            bufs = legal_depth(k)
            prm = draw_params(k) if rng.random() < P.p_per_frame else None
            pitch = 0 if host_d else pitch_option()
            le = st["last_exec"]
            if le is not None and not le.depth_host and rng.random() < P.p_again:
                # the last call once more (its frames usually refilled): a ready set lives for one call, matched or not
                bufs, prm, pitch, stream, host_d = le.bufs, le.params, le.pitch, le.stream, False
        if st["announced"] is not None and inexact and rtz and rng.random() < P.p_inexact_carrier:
            # a carrier outside the exact-division range: the set it leaves is refused by an exact call
            base = prm if prm is not None else (model.param,) * len(bufs)
            i = rng.randrange(len(base))
            twin = [p for p in inexact if p.zb(linear) == base[i].zb(linear)] or inexact
            prm = base[:i] + (rng.choice(twin),) + base[i + 1:]
        maybe_refill(bufs, pitch)
        outs = draw_outs(len(bufs))
        if len(outs) < len(bufs):                   # every AO buffer waits for a composite: let it run first
            emit(Op("comp_flush"))
            outs = draw_outs(len(bufs))
        op = Op("execute", bufs=bufs, outs=outs, params=prm, pitch=pitch, out_pitch=0 if host_o else pitch_option(),
                depth_host=host_d, out_host=host_o, stream=stream, read_debug=not P.free_running)
        emit(op)
        st.update(stream=stream, promised=st["announced"], announced=None, last_exec=op)
        loop, st["loop"] = st["loop"], None
        if loop is not None and any(c.ready is not None and c.ready.sized and c.ready.size == loop for c in (model.members if G else [model])):
            if not op.out_host and op.out_pitch == 0 and rng.random() < 0.3:
                do_comp_enqueue(1)                   # a composite waits across the resize: it runs plain, at the old size
            others = inside_sizes(other_than=cur_size())
            if len(others) > 1 and rng.random() < 0.12:
                loop = rng.choice([s for s in others if s != loop])      # the host changed its mind: the set is for another size
            do_resize(to=loop)                       # else the ready set the call left is for exactly this size: it stays
            if st["promised"] is not None and rng.random() < 0.7:
                st["honour"] = True
                do_execute()                         # the frames of the new size, as announced: the loop is closed
            return
        if P.reserve and st["promised"] is not None and st["promised"].size is None and one.cap != (0, 0) and rng.random() < 0.3:
            return do_resize()                       # an ordinary ready set and a resize: often one that ends at its size
        if P.w_reserve and not G and model.ready is not None and model.ready.sized and rng.random() < 0.2:
            return do_reserve(drop=True)             # (0, 0) while a sized ready set exists
        if prm is None and rng.random() < P.p_set_params_after:
            do_set_params(other_than=model.param)    # "as left by the last execute" is then not what the context holds

    def do_comp_enqueue(depth=0):
        le = st["last_exec"]
        if le is None or le.out_host or le.out_pitch != 0:      # composites take tightly packed DEVICE surfaces
            return do_execute()
        waiting = model.comp.color if not G and model.comp else ()
        free = [c for c in range(P.n_color) if c not in waiting]
        k = min(rng.randint(1, len(le.outs)), len(free) if not G else P.n_color // 2)
        half = P.n_color // 2                        # the pool: the two halves of the colour targets in turn, never one that waits
        colors = tuple(free[:k]) if not G else tuple(range(k) if st["flip"] else range(half, half + k))
        st["flip"] = not st["flip"]
        emit(Op("comp_enqueue", bufs=le.outs[:k], colors=colors, mode=rng.choice((0, 2))))
        r = rng.random()                             # what ends a wait other than the next call
        if depth == 0 and r < P.p_comp_ended_early:
            ender = rng.choice([lambda: emit(Op("comp_flush")), lambda: do_comp_enqueue(1), do_invalid, do_invalid] +
                               ([do_resize] if (not G and not P.free_running) or P.reserve else []) +
                               ([do_reserve] if P.w_reserve else []))
            ender()

    def sized_invalid(what):
        """The invalid calls of dynamic resolution that the state allows now; None: `what` is not among them."""
        cur, reserved = cur_size(), one.cap != (0, 0)
        beyond = [s for s in P.outside_sizes + ((one.cap[0] + 16, cur[1]),) if not one.within(*s)]
        inside = inside_sizes(other_than=cur)
        k = rng.randint(1, cap)
        if what == "sized_without_reservation" and not reserved:
            return Op("invalid", what=what, on="prefetch", bufs=legal_depth(k), size=rng.choice([s for s in P.sizes if s != cur]))
        if what == "sized_outside_reservation" and reserved:
            return Op("invalid", what=what, on="prefetch", bufs=legal_depth(k), size=rng.choice(beyond))
        if what == "sized_bad_pitch" and inside:
            return Op("invalid", what=what, on="prefetch", bufs=legal_depth(k), size=rng.choice(inside))
        if what == "reserve_below_current" and not P.free_running:     # (refused before anything synchronises, but keep the rule plain)
            return Op("invalid", what=what, on="reserve", size=rng.choice(((cur[0] - 8, cur[1]), (cur[0], cur[1] - 2), (8, 8))))
        if what == "pool_resize_uncovered" and G:
            st["uncovered"] = True
            return Op("invalid", what=what, on="resize", size=rng.choice(beyond))
        return None

    def do_invalid(what=None):
        if what is None and P.reserve and rng.random() < 0.5:
            what = rng.choice(SIZED_INVALID)
        if what is not None:
            op = sized_invalid(what)
            if op is not None:
                return emit(op)
        on = rng.choice(("execute", "prefetch"))
        kinds = ("n_zero", "n_over") + (("bad_params",) if bad else ())
        if not G:
            kinds += ("bad_pitch", "null_pointer")    # (the pool validates n and params[] itself before any member is given work)
        k = rng.randint(1, cap)
        what = rng.choice(kinds)
        emit(Op("invalid", what=what, on=on, bufs=legal_depth(k), outs=tuple(range(k)),
                params=tuple(bad[:1] * k) if what == "bad_params" else None, stream=st["stream"]))

    def do_set_params(other_than=None):
        emit(Op("set_params", param=rng.choice([p for p in valid if p != other_than])))
        st.update(promised=None, announced=None)

    def held(what):
        return any(getattr(c, what) is not None for c in (model.members if G else [model]))

    def do_resize(to=None):
        cur = (model.width, model.height)
        # an ordinary ready set waits for its call: the resizes that end at the size it was made for are the ones that count
        waits = st["promised"] is not None and st["promised"].size is None
        if to is None:
            if G or P.free_running:                  # only inside the reservation: the pool refuses others, and they synchronise
                sizes = inside_sizes(other_than=cur)
                if not sizes:
                    return
                to = rng.choice(sizes)
            else:
                to = rng.choice([s for s in P.sizes + P.outside_sizes if s != cur] or [cur])
            if P.reserve and one.within(*cur) and rng.random() < (0.3 if waits else 0.12):
                to = cur                             # a resize to the current size is a resize: it drops everything
        back = None
        if P.reserve and to != cur and one.within(*to) and one.within(*cur) and rng.random() < (0.4 if waits else 0.15):
            back = cur                               # there and back with no call in between: nothing survives it either
        emit(Op("resize", size=to))
        if back is not None:
            emit(Op("resize", size=back))
        # (what a resize keeps is still announced / promised: the next call is usually the one it was made for)
        stale = st["promised"] if to == cur or back is not None else None
        st.update(promised=st["promised"] if held("ready") else None, announced=st["announced"] if held("ann") else None,
                  last_exec=None, loop=None)
        if stale is not None and st["promised"] is None and rng.random() < 0.7:
            st.update(promised=stale, honour=True)   # the host asks for what it was promised all the same: a pass of its own
            do_execute()

    def do_reserve(drop=False):
        cur, c = cur_size(), one.cap
        grown = (max(P.reserve[0], c[0], cur[0]), max(P.reserve[1], c[1], cur[1]))
        if drop:
            size = (0, 0)
        elif c == (0, 0):
            size = grown
        else:
            r = rng.random()
            if r < 0.25:
                return do_invalid("reserve_below_current")
            size = (0, 0) if r < 0.6 else grown if r < 0.85 else (grown[0] + 16, grown[1] + 8)
        emit(Op("reserve", size=size))
        st.update(promised=None, announced=None, loop=None)

    def do_debug_set():
        key, values = rng.choice(DEBUG_KEYS)
        emit(Op("debug_set", key=key, value=rng.choice(values)))

    table = [(P.w_execute, do_execute), (P.w_prefetch, do_prefetch), (P.w_set_params, do_set_params),
             (P.w_comp_enqueue, do_comp_enqueue), (P.w_comp_flush, lambda: emit(Op("comp_flush"))), (P.w_invalid, do_invalid)]
    if not G:
        table.append((P.w_debug_set, do_debug_set))
        if not P.free_running:
            table.append((P.w_resize, do_resize))
    if P.reserve:
        if G or P.free_running:
            table.append((P.w_resize, do_resize))    # inside the reservation it synchronises nothing
        if not P.free_running:
            table.append((P.w_reserve, do_reserve))
            emit(Op("reserve", size=P.reserve))      # (a free-running sequence starts reserved: initial_cap)
    weights = [t[0] for t in table]
    while sum(op.kind != "refill" for op in ops) < P.length:
        if G and P.reserve and not st["uncovered"] and len(ops) >= P.length // 2:
            do_invalid("pool_resize_uncovered")      # once per sequence at the least
        if (st["announced"] is not None or st["promised"] is not None) and rng.random() < P.p_follow_up:
            do_execute()                             # an announcement is usually carried, a carried pass usually asked for
        else:
            rng.choices(table, weights)[0][1]()
    if ops[-1].kind != "execute":
        do_execute()                                 # end on a call, so that a carried pass or a waiting composite is seen
    return ops


def replay(ops, model):
    """[(op, expect)] through `model` (a fresh one): what the GPU tests hold the library to, and what the coverage tests count.
    For a PoolModel the expectation is the list of the members'."""
    return [(op, model.apply(op)) for op in ops]


def events_of(ops, model) -> List[str]:
    ev = []
    for _, e in replay(ops, model):
        for x in e if isinstance(e, list) else [e]:
            if x is not None:
                ev += x.events
    return ev


# ---- what the GPU tests commit to: parameter palette, cases and seeds (tests/test_call_model.py holds them to their coverage) -----

# camera (near, far, reversed_z, vertical fov) and AO properties of each palette entry.  Far planes are powers of two so that the
# linear-depth case can use them (include/meao.h: dist == z / far_clip exactly).  Entries 6 and 7 repeat the cameras of 0 and 2 with a
# tolerance outside the exact-division range (tests/helpers.py exact_range_edges: upsampleTolerance below about -13.2,
# noiseFilterTolerance above about 9); 8 is what meao_set_params rejects.
PALETTE_FIELDS = (
    dict(near=0.1, far=128.0, rev=True, fov=60.0, intensity=1.0, thickness=1.0, noise=0.0, blur=-4.6, upsample=-12.0),
    dict(near=0.25, far=128.0, rev=True, fov=45.0, intensity=1.7, thickness=2.5, noise=-3.0, blur=-2.0, upsample=-6.0),
    dict(near=0.1, far=64.0, rev=True, fov=75.0, intensity=0.6, thickness=1.0, noise=-8.0, blur=-8.0, upsample=-1.0),
    dict(near=0.1, far=128.0, rev=False, fov=60.0, intensity=2.0, thickness=7.0, noise=-1.0, blur=-4.6, upsample=-9.0),
    dict(near=0.1, far=128.0, rev=True, fov=90.0, intensity=0.0, thickness=10.0, noise=0.0, blur=-1.0, upsample=-12.0),
    dict(near=0.5, far=64.0, rev=False, fov=30.0, intensity=1.0, thickness=1.0, noise=-5.0, blur=-3.0, upsample=-3.0),
    dict(near=0.1, far=128.0, rev=True, fov=60.0, intensity=1.0, thickness=1.0, noise=0.0, blur=-4.6, upsample=-20.0, exact=False),
    dict(near=0.1, far=64.0, rev=True, fov=75.0, intensity=1.2, thickness=3.0, noise=20.0, blur=-4.6, upsample=-12.0, exact=False),
    dict(near=0.1, far=float("nan"), rev=True, fov=60.0, intensity=1.0, thickness=1.0, noise=0.0, blur=-4.6, upsample=-12.0,
         valid=False),
)
LINEAR_TAGS = (0, 4, 6)        # the linear-depth case: one camera (a linear frame is the Linearize of ITS camera's raw frame)


def palette(linear=False) -> List[Param]:
    return [Param(t, f["near"], f["far"], f["rev"], f.get("exact", True), f.get("valid", True))
            for t, f in enumerate(PALETTE_FIELDS) if not linear or t in LINEAR_TAGS or not f.get("valid", True)]


# config of each stepped / free-running case: depth format and AO storage by name, and what the model must know of them
CASES = {
    "r8_rtz_f32": dict(seed=7197),
    "f16_rtne_unorm16": dict(seed=9895, ao="f16", rtz=False, depth="unorm16"),
    "r8_rtz_linear_f32": dict(seed=5817, depth="linear_f32", linear=True),
    "r8_rtz_hq2": dict(seed=5151, hq_levels=2),
    "r8_rtz_not_pipelined": dict(seed=1145, pipelined=False),
}
FREE_CASES = {"r8_rtz_f32": dict(seed=6152), "r8_rtz_linear_f32": dict(seed=2640, depth="linear_f32", linear=True),
              "f16_rtne_unorm16": dict(seed=4401, ao="f16", rtz=False, depth="unorm16")}
POOL_CASES = {"pool2": dict(seed=301, members=2), "pool3": dict(seed=302, members=3)}

STEPPED = Profile()
FREE_RUNNING = Profile(free_running=True, length=48, sizes=((384, 256),), p_host=0.0, w_resize=0.0)
POOL = dict(length=40, max_batch=2, sizes=((384, 256),), p_host=0.0, p_other_stream=0.0, w_resize=0.0, w_debug_set=0.0, n_depth=12,
            n_out=14)


# Dynamic resolution (tests/test_dynamic_resolution_sequences_gpu.py): the reservation, four sizes inside it -- W % 8 == 0; one
# whose carried pass fits under the first; W % 8 != 0, the scalar forms; the reservation's own size -- and one outside that is
# wider but shorter, so that the reservation must grow to 416 x 272 and not to 416 x 200.
DYN_RESERVE = (400, 272)
DYN_SIZES = ((384, 256), (200, 120), (380, 250), (400, 272))
DYN_OUTSIDE = ((416, 200),)
DYN_STEPPED = Profile(sizes=DYN_SIZES, reserve=DYN_RESERVE, outside_sizes=DYN_OUTSIDE, w_resize=3.0, w_reserve=1.6, w_prefetch=8,
                      p_sized=0.6, p_sized_then_resize=0.6, p_ann_disturbed=0.3)
DYN_FREE = Profile(free_running=True, length=48, sizes=DYN_SIZES, reserve=DYN_RESERVE, p_host=0.0, w_resize=2.0, w_prefetch=8,
                   p_sized=0.6, p_sized_then_resize=0.7)
DYN_POOL = dict(POOL, sizes=DYN_SIZES[:3], reserve=DYN_RESERVE, outside_sizes=DYN_OUTSIDE, w_resize=2.5, w_prefetch=8, p_sized=0.6,
                p_sized_then_resize=0.65, n_depth=16)
DYN_CASES = {
    "r8_rtz_f32": dict(seed=4083),
    "f16_rtne_unorm16": dict(seed=3852, ao="f16", rtz=False, depth="unorm16"),
    "r8_rtz_linear_f32": dict(seed=4046, depth="linear_f32", linear=True),
    "r8_rtz_hq2": dict(seed=1024, hq_levels=2),
    "r8_rtz_not_pipelined": dict(seed=1111, pipelined=False),
}
DYN_FREE_CASES = {"r8_rtz_f32": dict(seed=2056), "r8_rtz_linear_f32": dict(seed=1939, depth="linear_f32", linear=True),
                  "f16_rtne_unorm16": dict(seed=2098, ao="f16", rtz=False, depth="unorm16")}
DYN_POOL_CASES = {"pool2": dict(seed=1068, members=2), "pool3": dict(seed=1046, members=3)}
DYN_POOL_FREE_SEEDS = {"pool2": 2387, "pool3": 1352}


def case_profile(kind: str, name: str):
    """(config, profile, seed) of a committed case: kind = stepped | free | pool_stepped | pool_free, or dyn_ + one of them."""
    dyn, base = kind.startswith("dyn_"), kind[4:] if kind.startswith("dyn_") else kind
    if base.startswith("pool"):
        c = (DYN_POOL_CASES if dyn else POOL_CASES)[name]
        # (free-running: a buffer is filled once, before its first use -- the pool's streams are its own, so a refill cannot be
        # ordered behind a member's work without the host synchronisation this mode is there to avoid)
        shape = dict(DYN_POOL, n_depth=48) if dyn and base == "pool_free" else DYN_POOL if dyn else POOL
        prof = Profile(pool=c["members"], free_running=base == "pool_free", p_refill=0.0 if base == "pool_free" else 0.7, **shape)
        seed = c["seed"] + (50 if base == "pool_free" else 0)
        if dyn and base == "pool_free":
            seed = DYN_POOL_FREE_SEEDS[name] + 50
    elif dyn:
        c = (DYN_CASES if base == "stepped" else DYN_FREE_CASES)[name]
        prof, seed = (DYN_STEPPED if base == "stepped" else DYN_FREE), c["seed"]
    else:
        c = (CASES if base == "stepped" else FREE_CASES)[name]
        prof, seed = (STEPPED if base == "stepped" else FREE_RUNNING), c["seed"]
    return c, prof, seed


def fresh_model(prof: Profile, cfg: dict):
    linear, rtz, pipelined = cfg.get("linear", False), cfg.get("rtz", True), cfg.get("pipelined", True)
    w, h = prof.sizes[0]
    pal = palette(linear)
    kw = dict(linear=linear, rtz=rtz, pipelined=pipelined, cap=initial_cap(prof))
    return PoolModel(prof.pool, w, h, prof.max_batch, pal[0], **kw) if prof.pool else ContextModel(w, h, prof.max_batch, pal[0], **kw)


def case_sequence(kind: str, name: str):
    """(ops, fresh model) of a committed case (kinds: case_profile)."""
    c, prof, seed = case_profile(kind, name)
    linear, rtz, pipelined = c.get("linear", False), c.get("rtz", True), c.get("pipelined", True)
    pal = palette(linear)
    ops = generate(seed, prof, pal, pal[0], linear=linear, rtz=rtz, pipelined=pipelined)
    return ops, fresh_model(prof, c)


def dynamic_sequences():
    """Every (kind, name) tests/test_dynamic_resolution_sequences_gpu.py adds."""
    out = [("dyn_stepped", n) for n in DYN_CASES] + [("dyn_free", n) for n in DYN_FREE_CASES]
    out += [(k, n) for k in ("dyn_pool_stepped", "dyn_pool_free") for n in DYN_POOL_CASES]
    return out


def committed_sequences():
    """Every (kind, name) the GPU tests run."""
    out = [("stepped", n) for n in CASES] + [("free", n) for n in FREE_CASES]
    out += [(k, n) for k in ("pool_stepped", "pool_free") for n in POOL_CASES]
    return out
