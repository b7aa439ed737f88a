"""The schedule of FrameStream (miniengineao_amd/stream_plan.py), checked as data: no GPU, no library, no torch.

A few hundred seeded random inputs -- 1 to 40 frames of the dynamic-resolution suite's sizes inside the capacity 400 x 272, row
strides, per-frame parameters and host / device location mixed at random, batch 1, 2 or 3 -- and on every plan the rules that
include/meao.h states for the pipelined loop.  "Context ops" below are the ops that reach the context: Announce, Execute, Resize.
Upload, WaitUploaded, Download and Yield touch streams, slots and the host only.

Look-ahead (invariant 5): when Yield(k) is emitted the planner has closed step k+2 and none later, so it has requested the
frames of the steps up to k+2 -- and one frame more exactly where step k+2 is not full and was ended by a frame that differs from
it.  That frame opens step k+3; a step that is not full cannot be known to have ended without it, and Execute(k+1), which has
to be submitted before the host waits for Download(k) if the two are to overlap, announces the closed step k+2.  The test asserts
both halves: never further than that, and never that one frame where step k+2 is full or the input ended behind it."""
import random

import pytest

from miniengineao_amd import stream_plan as P

SIZES = [(384, 256), (200, 120), (380, 250), (97, 61)]
CAPACITY = (400, 272)
A, B, C3 = (384, 256), (200, 120), (380, 250)
CONTEXT_OPS = (P.Announce, P.Execute, P.Resize)


def random_metas(rng):
    """Frames in runs of random length: within a run the size, stride, parameters and location stay, so that steps fill up."""
    metas = []
    n = rng.randint(1, 40)
    while len(metas) < n:
        w, h = rng.choice(SIZES)
        stride = rng.choice([w, w, 512])
        meta = (w, h, stride, rng.random() < 0.3, rng.choice([P.HOST, P.DEVICE]))
        metas += [meta] * rng.randint(1, 7)
    return metas[:n]


CASES = [(seed, batch) for seed in range(120) for batch in (1, 2, 3)]


class Recorded:
    """A metadata iterator that notes how many frames have been requested."""

    def __init__(self, metas):
        self.metas, self.requested = metas, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.requested >= len(self.metas):
            raise StopIteration
        self.requested += 1
        return self.metas[self.requested - 1]


def planned(metas, batch, size=None):
    """(ops, steps, frames requested before each op) through the incremental form."""
    src = Recorded(metas)
    planner = P.Planner(src, batch, CAPACITY, size=size)
    ops, seen = [], []
    for op in planner:
        ops.append(op)
        seen.append(src.requested)
    return ops, planner.steps, seen


def position(ops, op):
    assert ops.count(op) == 1, (op, ops.count(op))
    return ops.index(op)


@pytest.mark.parametrize("seed,batch", CASES)
def test_invariants_of_random_streams(seed, batch):
    rng = random.Random(seed * 7 + batch)
    metas = random_metas(rng)
    ops, steps, seen = planned(metas, batch)
    assert ops == P.plan(metas, batch, CAPACITY) and steps == P.steps_of(metas, batch, CAPACITY)
    last = len(steps) - 1

    # 1. every frame in exactly one step, in order; at most `batch` frames; uniform steps
    at = 0
    for k, s in enumerate(steps):
        assert s.index == k and s.first == at and 1 <= s.count <= batch
        for m in metas[s.first:s.first + s.count]:
            assert m == (s.width, s.height, s.stride, s.has_params, s.location)
        at += s.count
    assert at == len(metas)
    # (a step that is not full ended because the next frame differs, or the input did)
    for s in steps[:-1]:
        assert s.count == batch or metas[s.first + s.count] != metas[s.first]

    # 2. the context ops are exactly: [A(k+1) E(k) [R]] for every k, R exactly when the sizes differ and to the announced size
    want = []
    for k, s in enumerate(steps):
        if k < last:
            sized = steps[k + 1].size != s.size
            want.append(P.Announce(k + 1, sized))
        want.append(P.Execute(k))
        if k < last and sized:
            want.append(P.Resize(*steps[k + 1].size))
    ctx = [op for op in ops if isinstance(op, CONTEXT_OPS)]
    assert ctx == want
    for k in range(last):
        e = position(ops, P.Execute(k))
        assert isinstance(ops[e - 1], P.Announce) and ops[e - 1].step == k + 1             # directly in front of the carrying call
        if ops[e - 1].sized:
            assert ops[e + 1] == P.Resize(*steps[k + 1].size)                              # directly behind it
    assert not any(isinstance(op, P.Announce) and op.step == 0 for op in ops)

    # 3. host steps: Upload(k) < WaitUploaded(k) < Announce(k) < ... < Execute(k); slots
    held = {}                 # depth slot -> step that holds it (uploaded, not yet executed)
    results_live = {}         # result slot -> step (executed, not yet yielded)
    executed = set()
    for i, op in enumerate(ops):
        if isinstance(op, P.Upload):
            assert steps[op.step].host and op.slot == steps[op.step].depth_slot and 0 <= op.slot < 3
            assert op.slot not in held, (op, held)
            # the step that held the slot before was executed at least one call ago: the one running now reads other slots
            before = [s for s in steps[:op.step] if s.host and s.depth_slot == op.slot]
            if before:
                assert before[-1].index in executed and before[-1].index <= op.step - 3
            held[op.slot] = op.step
            assert len(held) <= 3
        elif isinstance(op, P.Execute):
            s = steps[op.step]
            executed.add(op.step)
            if s.host:
                assert held.pop(s.depth_slot) == op.step
                assert s.result_slot not in results_live
                results_live[s.result_slot] = op.step
                assert len(results_live) <= 2
            if op.step < last and steps[op.step + 1].host:                               # the announced frames are in their slot
                assert held.get(steps[op.step + 1].depth_slot) == op.step + 1
        elif isinstance(op, P.Yield) and steps[op.step].host:
            assert results_live.pop(steps[op.step].result_slot) == op.step
    assert not held and not results_live
    for k, s in enumerate(steps):
        if s.host:
            assert position(ops, P.Upload(k, s.depth_slot)) < position(ops, P.Execute(k))
            if k > 0:
                announce = [i for i, op in enumerate(ops) if isinstance(op, P.Announce) and op.step == k]
                assert len(announce) == 1
                assert position(ops, P.Upload(k, s.depth_slot)) < position(ops, P.WaitUploaded(k)) < announce[0]
        else:
            assert not any(isinstance(op, (P.Upload, P.WaitUploaded, P.Download)) and op.step == k for op in ops)

    # 4. Yield(k) follows Download(k) (host) / Execute(k) (device); in order; the download overlaps the next call
    yields = [op.step for op in ops if isinstance(op, P.Yield)]
    assert yields == list(range(len(steps)))
    for k, s in enumerate(steps):
        y = position(ops, P.Yield(k))
        if s.host:
            assert position(ops, P.Execute(k)) < position(ops, P.Download(k, s.result_slot)) < y
        else:
            assert position(ops, P.Execute(k)) < y
        if k < last:
            assert position(ops, P.Execute(k + 1)) < y          # the host waits for step k with step k+1 already submitted

    # 5. look-ahead
    for i, op in enumerate(ops):
        if isinstance(op, P.Yield):
            k = op.step
            through = steps[min(k + 2, last)]
            end = through.first + through.count                 # frames of the steps up to k+2
            early = k + 2 < last and through.count < batch      # step k+2 was ended by the first frame of step k+3
            assert seen[i] == end + (1 if early else 0), (k, seen[i], end, early)


def test_upload_is_issued_a_step_ahead_of_its_wait():
    """Uniform host stream: Upload(k+2) stands behind Execute(k) and in front of Execute(k+1), whose announcement waits for it;
    Download(k) stands between Execute(k) and Execute(k+1)."""
    ops = P.plan([(384, 256, 384, False, P.HOST)] * 12, 2, CAPACITY)
    for k in range(0, 3):
        assert position(ops, P.Execute(k)) < position(ops, P.Upload(k + 2, (k + 2) % 3)) < position(ops, P.WaitUploaded(k + 2)) \
            < position(ops, P.Execute(k + 1))
        assert position(ops, P.Execute(k)) < position(ops, P.Download(k, k % 2)) < position(ops, P.Execute(k + 1))


@pytest.mark.parametrize("seed,batch", [(s, b) for s in range(40) for b in (1, 2, 3)])
def test_frame_outside_the_capacity_raises_after_every_earlier_yield(seed, batch):
    rng = random.Random(1000 + seed * 7 + batch)
    metas = random_metas(rng)
    bad_at = rng.randrange(len(metas) + 1)
    bad = rng.choice([(401, 100), (100, 273), (0, 10), (4000, 4000)])
    stream = metas[:bad_at] + [bad + (bad[0], False, rng.choice([P.HOST, P.DEVICE]))] + metas[bad_at:]
    src = Recorded(stream)
    ops = []
    with pytest.raises(P.PlanError, match=f"frame {bad_at}:.*capacity.*max_size") as e:
        for op in P.Planner(src, batch, CAPACITY):
            ops.append(op)
    assert e.value.frame == bad_at and isinstance(e.value, ValueError)
    assert src.requested == bad_at + 1                        # nothing behind the refused frame was read
    # what was emitted is the complete plan of the frames in front of it: every one of them executed and yielded
    assert ops == P.plan(metas[:bad_at], batch, CAPACITY)
    assert [op.step for op in ops if isinstance(op, P.Yield)] == list(range(len(P.steps_of(metas[:bad_at], batch, CAPACITY))))
    with pytest.raises(P.PlanError) as e2:
        P.plan(stream, batch, CAPACITY)
    assert e2.value.ops == ops


def test_a_refusal_of_the_metadata_source_is_deferred_the_same_way():
    def source():
        yield 384, 256, 384, False, P.DEVICE
        yield 384, 256, 384, False, P.DEVICE
        yield 384, 256, 384, False, P.DEVICE
        raise ValueError("frame 3: wrong dtype")
    ops = []
    with pytest.raises(ValueError, match="frame 3: wrong dtype"):
        for op in P.Planner(source(), 2, CAPACITY):
            ops.append(op)
    assert ops == P.plan([(384, 256, 384, False, P.DEVICE)] * 3, 2, CAPACITY)


def test_empty_input_and_first_size():
    assert P.plan([], 2, CAPACITY) == []
    one = [(200, 120, 200, False, P.DEVICE)]
    assert P.plan(one, 2, CAPACITY) == [P.Execute(0), P.Yield(0)]
    assert P.plan(one, 2, CAPACITY, size=B) == [P.Execute(0), P.Yield(0)]
    assert P.plan(one, 2, CAPACITY, size=A) == [P.Resize(200, 120), P.Execute(0), P.Yield(0)]     # the context was left at another size


def test_the_order_of_the_dynamic_resolution_suite():
    """The size sequence of tests/test_dynamic_resolution_gpu.py::test_pipelined_stream_across_size_changes (A, B, A, C3, B, A, two
    frames each), whose loop drives by hand: announce(k+1) sized, execute(k), resize(size of k+1) -- and nothing behind the last."""
    sizes = [A, B, A, C3, B, A]
    for location in (P.DEVICE, P.HOST):
        ops = P.plan([(w, h, w, False, location) for (w, h) in sizes for _ in range(2)], 2, CAPACITY, size=A)
        by_hand = []
        for k in range(len(sizes)):
            if k + 1 < len(sizes):
                by_hand.append(P.Announce(k + 1, True))
            by_hand.append(P.Execute(k))
            if k + 1 < len(sizes):
                by_hand.append(P.Resize(*sizes[k + 1]))
        assert [op for op in ops if isinstance(op, CONTEXT_OPS)] == by_hand
        assert sum(isinstance(op, P.Resize) for op in ops) == 5


def test_the_module_needs_neither_torch_nor_the_library():
    import os
    import subprocess
    import sys
    code = ("import sys; import miniengineao_amd.stream_plan; "
            "bad = [m for m in ('torch', 'miniengineao_amd.stream', 'miniengineao_amd.ambient_occlusion') if m in sys.modules]; "
            "sys.exit(1 if bad else 0)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], cwd=root).returncode == 0
    with open(os.path.join(root, "miniengineao_amd", "stream_plan.py")) as fh:
        imports = [line.strip() for line in fh if line.startswith(("import ", "from "))]
    assert imports == ["from __future__ import annotations", "from typing import Iterable, Iterator, List, NamedTuple, Optional, Tuple"]
