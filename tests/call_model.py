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
Mixed-size batches (meao_execute_batch_extents; Op.extents) -- what the header left open and this model fixes:
  * `exact` of a mixed call is "every frame exact", as for every per-frame call: the context's parameters stand in for a frame
    without params[], the frames' sizes play no part.  The ready set the call promotes carries that `exact`.
  * The hostile mask after a mixed call has one bit per frame, in frame order, as after every call.
  * A ready set that a mixed call consumes is reported as refused for the one reason "mixed", also when every component of its key
    would have matched: the key is not compared.  ("mixed" is the last of KEY_COMPONENTS.)
  * meao_get_intermediate for a frame index >= n after a mixed call is refused, as after a uniform call.
  * A later meao_composite_enqueue* may name the outputs of a mixed call; the composite reads them tightly packed at the
    CONTEXT's size.  The generator therefore draws only AO buffers whose last writer was a frame of the context's size with packed
    rows (after a mixed call: the frames that happen to have the context's size and AO pitch option 0).
  * A pool member classifies ITS OWN share: a share whose extents all equal the member's size with one pair of strides is the
    pitched call for that member (it may reuse and carry inside its last kernel) while another member's share is mixed.
  * Uniform extents compare strides in texels: 0 and the packed row in bytes are the same stride.
"""
from __future__ import annotations

import dataclasses
import random
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

RING = 8                                           # meao.h: "a ring of 8 slots"
OK, ERR_INVALID_ARGUMENT = 0, -1
KEY_COMPONENTS = ("size", "pointer", "n", "stream", "pitch", "zb", "exact", "mixed")    # "mixed": consumed by a mixed call, key not compared
MAX_EXTENT = 32768                                 # meao.h: "outside [1, 32768]"
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
    from_mixed: bool = False                    # coverage only: a mixed call carried it


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
    mixed: bool = False                         # a mixed call: every frame has its own size and row strides
    sizes: Tuple[Tuple[int, int], ...] = ()     # per frame (the context's size at the time for every other call)
    rows: Tuple[Tuple[int, int], ...] = ()      # per frame: (depth, AO) row stride in texels


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
    # execute: meao_execute_batch_extents -- one (width, height, depth pitch option, AO pitch option) per frame, the options taken
    # at THAT frame's width; DEVICE / DEVICE.  invalid (MIXED_INVALID): the extents as the refused call passes them.
    # (In the repr only where it is set -- see below: the digests of the older sequences are taken over repr(ops).)
    extents: Optional[Tuple[Tuple[int, int, int, int], ...]] = field(default=None, repr=False)


# repr(Op) is what it was before Op.extents for every operation without extents (the pinned digests), and ends in the extents for
# an operation that has them, so that an assertion that prints a mixed call shows its sizes and pitch options.
_op_repr = Op.__repr__
Op.__repr__ = lambda self: _op_repr(self) if self.extents is None else "%s, extents=%r)" % (_op_repr(self)[:-1], self.extents)


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


# the invalid calls of mixed-size batches: each leaves announcement, ready set, waiting composite and last call as they were.
# extent_pitch_below_row: Op.key says which stride (0 depth, 1 AO), Op.value which frame.
MIXED_INVALID = ("extent_outside_capacity", "extent_zero", "extent_pitch_below_row", "extent_bad_params", "extent_n_over",
                 "extent_outside_on_one_member")


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
                       "carried_sized": 0, "kept_by_resize": 0, "mixed": 0, "carried_by_mixed": 0, "uniform_extents": 0}
        self.invalidated = False                    # coverage only: a reserve or resize took the last call away since it was made
        self.prev_stream = 0                        # coverage only: of the last execute, whatever happened since

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

    def invalid(self, op: Op, pool_checked=False) -> Expect:
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
        if op.what in MIXED_INVALID:
            if not pool_checked:                     # (the pool holds the call to its rule itself: n and the shares are the pool's)
                assert self._mixed_invalid_claim(op), ("illegal sequence: a mixed call claimed invalid that the library accepts", op)
            e.events.append("invalid_" + op.what)
            for what, x in (("announcement", self.ann), ("ready", self.ready), ("composite", self.comp)):
                if x is not None:
                    e.events.append("mixed_refused_keeps_" + what)
        if self.ann is not None:
            e.events.append("invalid_while_announced")
        if self.comp is not None:
            e.events.append("invalid_while_composite")
        if self.readable():
            e.events.append("debug_read_after_invalid")
            if self.last.mixed:
                e.events.append("mixed_then_debug_read")
        return e

    def _mixed_invalid_claim(self, op: Op, limit=None) -> bool:
        """The generator's claim that a mixed call is invalid, held to the rule it names: that rule refuses it, and nothing before
        it in the validation order does."""
        n, ext = len(op.bufs), op.extents
        ok_n = 1 <= n <= (self.max_batch if limit is None else limit)
        rows = None
        if op.what == "extent_n_over":
            return not ok_n
        if op.what == "extent_pitch_below_row":      # the driver passes one stride of width - 1 texels: frame op.value, kind op.key
            rows = [list(r) for r in self.extent_rows(ext)]
            rows[op.value][op.key] = ext[op.value][0] - 1
            ext_ok = self.check_extents(n, ext, op.params, None, limit) == OK
            return ok_n and ext_ok and self.check_extents(n, ext, op.params, rows, limit) != OK
        if op.what == "extent_bad_params":
            return ok_n and op.params is not None and self.check_extents(n, ext, None, None, limit) == OK and \
                self.check_extents(n, ext, op.params, None, limit) != OK
        cw, ch = self.capacity()
        bad = [(w, h) for w, h, _, _ in ext if not (1 <= w <= cw and 1 <= h <= ch)]
        if op.what == "extent_zero":
            return ok_n and len(bad) == 1 and 0 in bad[0]
        return ok_n and len(bad) == 1 and min(bad[0]) >= 1       # extent_outside_capacity (for the pool: on one member)

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

    def capacity(self) -> Tuple[int, int]:
        """'The capacity is the reservation (meao_reserve) where the context holds one, else the context's size'"""
        return self.cap if self.cap != (0, 0) else (self.width, self.height)

    def extent_rows(self, extents, rows=None):
        """Per frame (depth, AO) row strides in texels: given outright (the model's own tests, the one illegal stride of a
        sequence) or from the pitch options at each frame's own width."""
        return tuple(rows) if rows is not None else tuple((row_texels(dp, w), row_texels(ap, w)) for w, h, dp, ap in extents)

    def check_extents(self, n, extents, params=None, rows=None, limit=None) -> int:
        """The validation of meao_execute_batch_extents, in the header's order: n and params[] as meao_execute_batch_params checks
        them, then every frame's size against [1, 32768] and the capacity, then each pitch against its own frame."""
        if not 1 <= n <= (self.max_batch if limit is None else limit) or len(extents) != n:
            return ERR_INVALID_ARGUMENT
        if params is not None and not all(p.valid for p in params):
            return ERR_INVALID_ARGUMENT
        cw, ch = self.capacity()
        for (w, h, _, _), (drow, arow) in zip(extents, self.extent_rows(extents, rows)):
            if not (1 <= w <= MAX_EXTENT and 1 <= h <= MAX_EXTENT) or w > cw or h > ch:
                return ERR_INVALID_ARGUMENT
            if drow < w or arow < w:
                return ERR_INVALID_ARGUMENT
        return OK

    def extents_uniform(self, extents, rows=None) -> bool:
        """'every extent equals the context's size and all frames share their pitches' (strides compared in texels)"""
        r = self.extent_rows(extents, rows)
        return all((w, h) == (self.width, self.height) for w, h, _, _ in extents) and len(set(r)) == 1

    def execute_extents(self, bufs, outs, extents, params=None, stream=0, rows=None) -> Expect:
        """meao_execute_batch_extents.  A refused call changes nothing; uniform extents ARE the pitched call; every other call is
        a mixed call."""
        n = len(bufs)
        if len(outs) != n or self.check_extents(n, extents, params, rows) != OK:
            return self._expect(status=ERR_INVALID_ARGUMENT)
        r = self.extent_rows(extents, rows)
        if self.extents_uniform(extents, rows):
            had_ready, had_ann = self.ready is not None, self.ann is not None
            e = self._execute(bufs, outs, params, stream=stream, depth_rows=r[0][0], out_rows=r[0][1])
            self.totals["uniform_extents"] += 1
            e.events.append("uniform_extents")
            if e.reused:
                e.events.append("uniform_extents_reuses")
            if had_ann:
                e.events.append("uniform_extents_carries")
            return e
        prm = tuple(params) if params is not None else (self.param,) * n
        exact = self._exact(prm)                    # "every frame exact", as for every per-frame call
        e = Expect(launched=True, exact=exact, own_pass=True, per_frame=True)
        e.events.append("mixed_call")
        if any(b in self.fresh for b in bufs):
            e.events.append("refilled_before_call")
        if self.last is None and self.invalidated:
            e.events.append("mixed_after_invalidation")
        if stream != self.prev_stream:
            e.events.append("mixed_on_other_stream")
        # a waiting composite runs first as plain launches, also when the call has no params[]
        if self.comp is not None:
            self._run_comp_plain(e, "mixed_call")
            e.events.append("mixed_flushes_composite")
        # a ready set is consumed unmatched: its key is not compared
        had_ready = self.ready is not None
        if had_ready:
            e.refused = ("mixed",)
            e.events.append("mixed_consumes_ready")
            if tuple(bufs) == self.ready.bufs and stream == self.ready.stream:
                e.events.append("mixed_consumes_ready_same_buffers")
        self.ready = self.dropped = None
        # an announcement of any kind is carried, as a launch of its own, and promoted as usual
        a = self.ann
        if a is not None:
            e.carried = a
            aprm = a.params if a.params is not None else (self.param,) * len(a.bufs)
            self.ready = ReadySet(a.bufs, stream, a.pitch, tuple(p.zb(self.linear) for p in aprm), exact, a.sized,
                                  a.size if a.sized else (self.width, self.height), from_mixed=True)
            self.ann = None
            self.totals["carried_by_mixed"] += 1
            kinds = [k for k, is_k in (("sized", a.sized), ("per_frame", a.params is not None), ("pitched", a.pitch != a.size[0])) if is_k]
            e.events += ["mixed_carries_" + k for k in kinds or ["plain"]]
            if a.sized:
                self.totals["carried_sized"] += 1
                e.events.append("sized_carried")
            if len(a.bufs) > n:
                self.totals["carried_more"] += 1
                e.events.append("mixed_carries_more_frames_than_n")
        if params is None and (a is None or a.params is None):
            e.events.append("mixed_shared_params_takes_ring_slot")
        self.ring = (self.ring + 1) % RING
        self.totals["per_frame"] += 1
        for b in bufs:
            self.fresh.discard(b)
        self.last = LastCall(n, prm, tuple(bufs), tuple(outs), -1, -1, False, False, stream, exact, False, had_ready, params is None,
                             True, tuple((w, h) for w, h, _, _ in extents), r)
        self.last_intact, self.invalidated, self.prev_stream = True, False, stream
        self.totals["own"] += 1
        self.totals["mixed"] += 1
        self.totals["carried"] += a is not None
        e.last_valid = True
        return e

    def execute(self, bufs, outs, params=None, pitch=0, out_pitch=0, depth_host=False, out_host=False, stream=0) -> Expect:
        return self._execute(bufs, outs, params, pitch, out_pitch, depth_host, out_host, stream)

    def _execute(self, bufs, outs, params=None, pitch=0, out_pitch=0, depth_host=False, out_host=False, stream=0, depth_rows=None,
                 out_rows=None) -> Expect:
        """depth_rows / out_rows: the row strides in texels given outright (uniform extents), instead of the pitch options."""
        n = len(bufs)
        assert 1 <= n <= self.max_batch and len(outs) == n
        prm = tuple(params) if params is not None else (self.param,) * n
        exact = self._exact(prm)
        depth_pitch = self.width if depth_host else self.pitch_texels(pitch)      # HOST frames are staged packed
        if depth_rows is not None:
            depth_pitch = depth_rows
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
        out_texels = self.width if out_host else self.pitch_texels(out_pitch) if out_rows is None else out_rows
        self.last = LastCall(n, prm, tuple(bufs), tuple(outs), depth_pitch, out_texels, depth_host, out_host, stream, exact, e.reused,
                             r is not None, params is None, False, ((self.width, self.height),) * n, ((depth_pitch, out_texels),) * n)
        self.last_intact, self.invalidated, self.prev_stream = True, False, stream
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
            if self.last.mixed:
                e.events.append("mixed_then_debug_read")
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
                if what == "ready" and x.from_mixed:
                    e.events.append("sized_ready_from_mixed_kept_by_resize")
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
        self._invalidate_last(e)
        e.comp_pending = 0
        return e

    def _invalidate_last(self, e: Expect) -> None:
        """A reserve or a resize: nothing "as left by the last execute" is left, per-frame sizes included."""
        if self.last is not None:
            self.invalidated = True
            if self.last.mixed:
                e.events.append("mixed_then_reserve_invalidates")
        self.last = None

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
        self.ann = self.ready = self.dropped = None                 # the buffers moved: nothing "as left by the last execute" is left
        self._invalidate_last(e)
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
            if self.last.mixed:
                e.events.append("mixed_then_debug_read")
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
        if k == "execute" and op.extents is not None:
            e = self.execute_extents(op.bufs, op.outs, op.extents, op.params, op.stream)
            assert e.status == OK, ("illegal sequence: a mixed call the library refuses", op)
            if op.read_debug and self.last.mixed:
                e.events.append("mixed_then_debug_read")
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

    def check_extents(self, op: Op, claimed=False) -> int:
        """meao_pool_execute_batch_extents: n against max_batch x members, then every member's share by that member's rules, before
        any member is given work.  claimed: an invalid Op -- the rule it names must be the one that refuses it."""
        n = len(op.bufs)
        if claimed and op.what == "extent_n_over":
            return OK if 1 <= n <= self.max_batch * self.G else ERR_INVALID_ARGUMENT
        if not 1 <= n <= self.max_batch * self.G:
            assert not claimed, op
            return ERR_INVALID_ARGUMENT
        bad = 0
        for m, c in enumerate(self.members[:n]):
            sub = dataclasses.replace(op, bufs=self.share(m, op.bufs), extents=self.share(m, op.extents),
                                      params=None if op.params is None else self.share(m, op.params))
            if claimed:
                if op.what == "extent_pitch_below_row":
                    mine = op.value % self.G == m
                    sub.value = op.value // self.G
                    ok = c._mixed_invalid_claim(sub) if mine else c.check_extents(len(sub.bufs), sub.extents, sub.params) == OK
                    bad += mine and ok
                    assert ok, op
                elif op.what == "extent_bad_params":
                    bad += c._mixed_invalid_claim(sub)
                else:
                    refused = c.check_extents(len(sub.bufs), sub.extents, sub.params) != OK
                    assert not refused or c._mixed_invalid_claim(sub), op
                    bad += refused
            elif c.check_extents(len(sub.bufs), sub.extents, sub.params) != OK:
                return ERR_INVALID_ARGUMENT
        if claimed:
            if op.what == "extent_outside_on_one_member":
                assert bad == 1, op                   # one member's share is refused, the others' are fine: still nobody runs
            return ERR_INVALID_ARGUMENT if bad else OK
        return OK

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
                                      params=None if op.params is None else self.share(m, op.params),
                                      extents=None if op.extents is None else self.share(m, op.extents))
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
            kinds = None
            if op.extents is not None:
                # "Every member's share is validated against that member's capacity before any member enqueues"
                assert self.check_extents(op) == OK, ("illegal sequence: a mixed pool call the library refuses", op)
                kinds = [c.extents_uniform(self.share(m, op.extents)) for m, c in enumerate(self.members[:n])]
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
            if kinds is not None and not all(kinds):
                if any(kinds):                       # each member classifies its own share
                    ev.append("pool_member_uniform_while_other_mixed")
                    if any(u and x.reused for u, x in zip(kinds, out)):
                        ev.append("pool_member_uniform_reuses_while_other_mixed")
                if n < self.G:
                    ev.append("pool_mixed_idle_member")
            return out
        if k == "prefetch":
            self.announced_n = len(op.bufs)
            return self._deal(op, lambda c: c.drop_announcement(False))
        if k == "comp_enqueue":
            return self._deal(op)
        if k == "invalid":
            if op.what in MIXED_INVALID:
                assert self.check_extents(op, claimed=True) != OK, ("illegal sequence: a mixed pool call claimed invalid", op)
            out = [c.invalid(op, pool_checked=True) for c in self.members]
            if op.what in MIXED_INVALID:
                out[0].events.append("pool_mixed_refused_whole")
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
    # mixed-size batches (meao_execute_batch_extents); the defaults draw nothing of them, and no random number for them
    p_mixed: float = 0.0               # share of executes that are mixed calls
    p_uniform_extents: float = 0.0     # share of the other DEVICE / DEVICE executes that go through the extents call, all frames alike
    mixed_sizes: Tuple[Tuple[int, int], ...] = ()     # the sizes a mixed call's frames draw from (those inside the capacity)

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

    def fits(size):
        cw, ch = one.capacity()
        return size[0] <= cw and size[1] <= ch

    def frame_depth(size, pitch, avoid):
        """(buffer, fillable) for one frame of a mixed call: one that holds a frame of `size` under `pitch` or may be given one
        now; failing that any other, read under the frame's own size and stride whatever was laid out in it."""
        once = bool(G) and P.free_running
        ok = [b for b in range(P.n_depth) if b not in avoid and
              (laid.get(b) == (size, pitch) or (not model.referenced(b) and not (once and b in model.contents)))]
        if ok:
            return rng.choice(ok), True
        return rng.choice([b for b in range(P.n_depth) if b not in avoid]), False

    def do_mixed_execute():
        """meao_execute_batch_extents with frames that are not all the context's size; False: no such sizes fit the capacity."""
        cur = cur_size()
        sizes_in = [s for s in P.mixed_sizes if fits(s)]
        others = [s for s in sizes_in if s != cur]
        if not others:
            return False
        stream, promised = st["stream"], st["promised"]
        same = promised is not None and held("ready") and rng.random() < 0.4
        if same:
            bufs = promised.bufs                     # the ready set's own buffers, so that "mixed" is all that refuses it
        else:
            bufs = None
            if not G and rng.random() < max(P.p_other_stream, 0.25):
                stream = 1 - stream
        n = len(bufs) if same else rng.randint(1, cap)
        ext = [list(rng.choice(sizes_in)) + [pitch_option(), pitch_option()] for _ in range(n)]
        if G and n > 1 and rng.random() < 0.5:
            # one member's share alike at the members' size (with the announced stride where the frames are the announced ones):
            # that member makes the pitched call, and may reuse, while the others make mixed calls
            m = rng.randrange(min(G, n))
            for f in range(m, n, G):
                ext[f] = [cur[0], cur[1], promised.pitch if same and promised.size is None and promised.pitch != 3 else 0, 0]
        if all(tuple(x[:2]) == cur for x in ext):
            f = rng.randrange(n)
            ext[f][:2] = rng.choice(others)
        if not same:
            chosen = []
            for w, h, dp, _ in ext:
                b, fillable = frame_depth((w, h), dp, chosen)
                if fillable:
                    maybe_refill((b,), dp, (w, h))
                chosen.append(b)
            bufs = tuple(chosen)
        prm = draw_params(n) if rng.random() < P.p_per_frame else None
        outs = draw_outs(n)
        if len(outs) < n:
            emit(Op("comp_flush"))
            outs = draw_outs(n)
        op = Op("execute", bufs=tuple(bufs), outs=outs, params=prm, stream=stream, read_debug=not P.free_running,
                extents=tuple(tuple(x) for x in ext))
        emit(op)
        after_execute(op, prm, stream)
        return True

    def do_execute():
        if P.p_mixed and not st.get("honour", False) and rng.random() < P.p_mixed and do_mixed_execute():
            return
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
        # (three times as often where the call asks for what it was promised: the extents call must reuse as the pitched call does)
        if P.p_uniform_extents and not host_d and not host_o and not (pitch == 3 and model.width > PITCH_FIXED) and \
                rng.random() < P.p_uniform_extents * (3 if promised is not None and r < P.p_honour else 1):
            # the extents call with every frame alike at the context's size: the pitched call in every respect
            op.extents = ((model.width, model.height, op.pitch, op.out_pitch),) * len(bufs)
        emit(op)
        after_execute(op, prm, stream)

    def after_execute(op, prm, stream):
        st.update(stream=stream, promised=st["announced"], announced=None, last_exec=op)
        if P.p_mixed and st["promised"] is not None and rng.random() < 0.15:
            do_invalid(rng.choice(MIXED_INVALID))    # a refused mixed call while a ready set waits: it stays
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
        if le is not None and le.extents is not None and not one.extents_uniform(le.extents):
            # after a mixed call: the frames that have the context's size and packed AO rows, in the pool the leading ones (frame
            # k of the composite goes to member k mod G, which must be the member that produced it)
            ok = [x[:2] == cur_size() and x[3] == 0 for x in le.extents]
            lead = ok.index(False) if False in ok else len(ok)
            elig = tuple(o for o, good in zip(le.outs, ok) if good) if not G else le.outs[:lead]
            if not elig:
                return do_execute() if depth == 0 else None
            le = dataclasses.replace(le, outs=elig)
        if le is None or le.out_host or le.out_pitch != 0:      # composites take tightly packed DEVICE surfaces
            return do_execute()
        waiting = model.comp.color if not G and model.comp else ()
        free = [c for c in range(P.n_color) if c not in waiting]
        k = min(rng.randint(1, len(le.outs)), len(free) if not G else P.n_color // 2)
        half = P.n_color // 2                        # the pool: the two halves of the colour targets in turn, never one that waits
        colors = tuple(free[:k]) if not G else tuple(range(k) if st["flip"] else range(half, half + k))
        st["flip"] = not st["flip"]
        emit(Op("comp_enqueue", bufs=le.outs[:k], colors=colors, mode=rng.choice((0, 2))))
        if P.p_mixed and depth == 0 and rng.random() < P.p_mixed:
            if rng.random() < 0.3:
                do_invalid(rng.choice(MIXED_INVALID))      # a refused mixed call leaves the batch waiting ...
            if do_mixed_execute():                   # ... and a mixed call runs it first as plain launches, params[] or not
                return
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

    def mixed_invalid(what):
        """A mixed call the library must refuse for the rule `what` names and no other; None: not possible now."""
        sizes_in = [s for s in P.mixed_sizes if fits(s)]
        n = cap + 1 if what == "extent_n_over" else rng.randint(1, cap)
        if not sizes_in or (what == "extent_outside_on_one_member" and (not G or n < 2)) or (what == "extent_bad_params" and not bad):
            return None
        cw, ch = one.capacity()
        ext = [list(rng.choice(sizes_in)) + [pitch_option(), pitch_option()] for _ in range(n)]
        f = rng.randrange(n)
        prm, key = None, 0
        if what in ("extent_outside_capacity", "extent_outside_on_one_member"):
            ext[f][:2] = rng.choice(((cw + 16, ext[f][1]), (ext[f][0], ch + 8)))
        elif what == "extent_zero":
            ext[f][rng.randrange(2)] = 0
        elif what == "extent_bad_params":
            prm = tuple(bad[0] if i == f else rng.choice(valid) for i in range(n))
        elif what == "extent_pitch_below_row":
            key = rng.randrange(2)                   # the depth stride or the AO stride of frame f: one texel short of its row
        elif rng.random() < P.p_per_frame:
            prm = draw_params(n)
        return Op("invalid", what=what, on="execute", bufs=legal_depth(min(n, P.n_depth)), outs=tuple(range(n)), params=prm,
                  stream=st["stream"], extents=tuple(tuple(x) for x in ext), key=key, value=f)

    def do_invalid(what=None):
        if what is None and P.p_mixed and rng.random() < 0.5:
            what = rng.choice(MIXED_INVALID)
        if what in MIXED_INVALID:
            op = mixed_invalid(what)
            if op is not None:
                return emit(op)
            what = None
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


def header_lets_it_ride(a: Announcement, n: int, size, f32_depth: bool) -> bool:
    """What include/meao.h names as needed for an announced pass to run INSIDE the last kernel of a carrier that is not a mixed
    call (meao_prefetch_batch, meao_prefetch_batch_sized): f32 depth, the announced width % 8 == 0 under a stride of whole
    4-texel vectors (aligned frames are the driver's: every surface is), no more frames than the carrier's n, and
    ceil(w / 128) x ceil(h / 32) announced tiles within the carrier's ceil(W / 64) x ceil(H / 64).  Necessary, not sufficient:
    "host code decides".  The model predicts nothing from it; the free-running tests bound the fused launches of a trace by it."""
    (w, h), up = a.size, lambda x, t: -(-x // t)
    return f32_depth and w % 8 == 0 and a.pitch % 4 == 0 and len(a.bufs) <= n and \
        up(w, 128) * up(h, 32) <= up(size[0], 64) * up(size[1], 64)


def may_ride_count(ops, model, f32_depth=True) -> int:
    """The carried passes of a sequence that the header lets ride (never one a mixed call carries), over all members."""
    count = 0
    for op in ops:
        e = model.apply(op)
        if op.kind == "execute":
            members = model.members if isinstance(e, list) else [model]
            for m, x in enumerate(e if isinstance(e, list) else [e]):
                if x is not None and x.carried is not None and "mixed_call" not in x.events:
                    count += header_lets_it_ride(x.carried, len(op.bufs[m::len(members)]), (members[m].width, members[m].height), f32_depth)
    return count


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


# Mixed-size batches (tests/test_mixed_size_sequences_gpu.py): the dynamic-resolution profiles, whose executes are now often mixed
# calls.  The frames draw from the four sizes the context moves between and from four more, the smallest shapes that still have one
# tile in every pass: an odd width, a frame taller but narrower than another (97 x 61 against 129 x 65 and 257 x 31), one wider but
# shorter.
MIX_SIZES = DYN_SIZES + ((33, 17), (97, 61), (129, 65), (257, 31))
MIX = dict(p_mixed=0.4, p_uniform_extents=0.1, mixed_sizes=MIX_SIZES)
MIX_STEPPED = dataclasses.replace(DYN_STEPPED, length=44, **MIX)
MIX_FREE = dataclasses.replace(DYN_FREE, length=44, **MIX)
MIX_POOL = dict(DYN_POOL, max_batch=4, n_depth=20, n_out=26, **MIX)
MIX_CASES = {name: dict(c, seed=seed) for (name, c), seed in zip(CASES.items(), (166, 349, 324, 16, 92))}
MIX_FREE_CASES = {name: dict(c, seed=seed) for (name, c), seed in zip(FREE_CASES.items(), (545, 722, 38))}
MIX_POOL_CASES = {"pool2": dict(seed=7, members=2), "pool3": dict(seed=90, members=3)}
MIX_POOL_FREE_SEEDS = {"pool2": 147, "pool3": 333}


def case_profile(kind: str, name: str):
    """(config, profile, seed) of a committed case: kind = stepped | free | pool_stepped | pool_free, or dyn_ / mix_ + one of them."""
    if kind.startswith("mix_"):
        base = kind[4:]
        if base.startswith("pool"):
            c = MIX_POOL_CASES[name]
            free = base == "pool_free"
            shape = dict(MIX_POOL, n_depth=64) if free else MIX_POOL
            prof = Profile(pool=c["members"], free_running=free, p_refill=0.0 if free else 0.7, **shape)
            return c, prof, MIX_POOL_FREE_SEEDS[name] if free else c["seed"]
        c = (MIX_CASES if base == "stepped" else MIX_FREE_CASES)[name]
        return c, (MIX_STEPPED if base == "stepped" else MIX_FREE), c["seed"]
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


def mixed_sequences():
    """Every (kind, name) tests/test_mixed_size_sequences_gpu.py adds."""
    out = [("mix_stepped", n) for n in MIX_CASES] + [("mix_free", n) for n in MIX_FREE_CASES]
    out += [(k, n) for k in ("mix_pool_stepped", "mix_pool_free") for n in MIX_POOL_CASES]
    return out


def committed_sequences():
    """Every (kind, name) the GPU tests run."""
    out = [("stepped", n) for n in CASES] + [("free", n) for n in FREE_CASES]
    out += [(k, n) for k in ("pool_stepped", "pool_free") for n in POOL_CASES]
    return out
