"""Mixed-size batches on the GPU (meao_execute_batch_extents): one size per frame inside the context's capacity.

A context of 400 x 272, max_batch 8.  The result and every valid debug buffer of EVERY frame of a mixed call are compared, NaN-aware,
with the CPU oracle run at that frame's own size and parameters (oracle.run with the frame's Settings), and every output surface
lies inside a sentinel-filled allocation whose other bytes must come back untouched.  A frame's contents depend on its size and
a seed only, so the orderings and the launch-structure variants share one oracle run per frame.

Sizes: (33, 17) has one tile in every pass of every tiling; 400 x 272 is the capacity; the "tile edge" list sits on and one past
the 64 / 128 / 256 texel tile widths and the 32 / 64 row tile heights of the passes."""
import dataclasses

import numpy as np
import pytest

from miniengineao_amd import _lib as L
from tests import helpers as H
from tests.helpers import colour, want_of
from tests.mixed_size import (
    COLUMNS, CTX, EDGES, F32, FAMILIES, FUSED, MAX_BATCH, MixedCall, ORDER, ORDERINGS, SENTINEL, VARIANTS, base_settings,
    context, frame, frame_settings, run_variant)

pytestmark = pytest.mark.gpu

# ---- orderings, tile edges, capacity

@pytest.mark.parametrize("order", sorted(ORDERINGS))
@pytest.mark.parametrize("per_frame", [False, True])
def test_orderings(oracle, order, per_frame):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        call = MixedCall(torch, oracle, base, ORDERINGS[order], per_frame=per_frame)
        call.execute(ao)
        call.check(ao, what=order)
        # the view of a buffer has the frame's own size too
        f = ORDERINGS[order].index((97, 61))
        view = ao.debug_view(10, frame=f)
        assert view.shape == (61, 97) and np.array_equal(view, oracle.debug_view(call.want(f), 10, call.settings[f]))
    finally:
        ao.close()


def test_tile_edges(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        call = MixedCall(torch, oracle, base, EDGES, per_frame=True)
        call.execute(ao)
        call.check(ao, what="edges")
    finally:
        ao.close()


def test_capacity_is_the_reservation(oracle):
    """The same sizes inside meao_reserve(400, 272) on a context currently resized to 200 x 120: the capacity bounds them, the
    context's size is neither read nor changed."""
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        ao.reserve(*CTX)
        ao.resize(200, 120)
        for sizes in (ORDER, EDGES):
            call = MixedCall(torch, oracle, base, sizes)
            call.execute(ao)
            call.check(ao, what="reserved")
        assert (ao.width, ao.height) == (200, 120) and ao.capacity == CTX
        # a uniform call at the context's own size afterwards
        after = MixedCall(torch, oracle, base, [(200, 120)] * 2)
        ao.execute_device([d.ptr for d in after.depth], [o.ptr for o in after.out])
        after.check(ao, debug_buffers=False, what="uniform at 200 x 120")
    finally:
        ao.close()


# ---- every guarded kernel, under mixed sizes

@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_launch_structures_and_configurations(oracle, name):
    import torch
    run_variant(torch, oracle, name)


@pytest.mark.parametrize("column", sorted(set(COLUMNS) - {"r8_rtz_exact"}))
def test_other_columns(oracle, column):
    import torch
    run_variant(torch, oracle, "defaults", column=column)


TRACE_CHILD = r"""
import sys
import torch
from oracle import oracle as O
from tests import mixed_size as M
O.build()
for name in sorted(M.VARIANTS):
    M.run_variant(torch, O, name, debug_buffers=False)
print("mixed-size trace child ok")
"""


def test_every_per_frame_kernel_family_runs_in_a_mixed_call(tmp_path):
    """The child makes mixed calls only (R8 / RTZ / exact column): every *_frames family except the fused last kernel must show
    in its trace, each variant's own kernels by name, and no kernel of the shared calls."""
    k = H.kernel_trace(tmp_path, TRACE_CHILD)
    assert "mixed-size trace child ok" in k.stdout
    for family in FAMILIES:
        assert k[family] > 0, (family, k.short)
    assert k[FUSED] == 0 and k["upsample_final_with_next_downsample_kernel"] == 0
    for shared in ("downsample_kernel", "render_kernel", "render_small_kernel", "upsample_kernel", "upsample_final_kernel",
                   "upsample_final_small_kernel", "upsample_three_level_kernel", "upsample_two_level_kernel"):
        assert k[shared] == 0, (shared, k.short)
    from tests import kernel_inventory as K
    cols = {K.column_of(n) for n in k.short if K.column_of(n) and K.column_of(n)[0] != "ds"}
    assert cols == {("0", "false", "0")}, cols


# ---- the call's launch shape

def l1_tiles(sizes):
    """64 x 32 tiles of the L2 -> L1 pass, summed over the frames."""
    half = lambda v: (v + 1) // 2
    return sum(((half(w) + 63) // 64) * ((half(h) + 31) // 32) for w, h in sizes)


THRESHOLD_CHILD = r"""
import sys
import torch
from oracle import oracle as O
from miniengineao_amd import _lib as L
from tests import mixed_size as M
O.build()
base = M.base_settings(O)
for limit in (int(sys.argv[1]), int(sys.argv[1]) - 1):
    ao = M.context(base, debug={L.DEBUG_NESTED_MAX_TILES: limit})
    call = M.MixedCall(torch, O, base, M.ORDER)
    call.execute(ao)
    call.check(ao, debug_buffers=False)
    ao.close()
print("threshold child ok")
"""


def test_thresholds_compare_the_sum_over_the_frames(tmp_path):
    total = l1_tiles(ORDER)
    assert total == 1 + 4 * 5 + 2 * 2 + 1 * 1 and total != len(ORDER) * l1_tiles(ORDER[:1]) and total != len(ORDER) * l1_tiles([CTX])
    k = H.kernel_trace(tmp_path, THRESHOLD_CHILD, [str(total)])
    assert "threshold child ok" in k.stdout
    # NESTED_MAX_TILES = the sum: the three-level launch; one less: the two-level launch and L2 -> L1 on its own
    assert k["upsample_three_level_frames_kernel"] == 1 and k["upsample_two_level_frames_kernel"] == 1, k.short


VECTOR_CHILD = r"""
import torch
from oracle import oracle as O
from tests import mixed_size as M
O.build()
base = M.base_settings(O)
ao = M.context(base)
for sizes in (M.ALIGNED, M.ALIGNED[:3] + [(97, 61)]):
    call = M.MixedCall(torch, O, base, sizes)
    call.execute(ao)
    call.check(ao, debug_buffers=False)
ao.close()
print("vector child ok")
"""


def test_vector_forms_need_every_frame_eligible(tmp_path):
    from tests import kernel_inventory as K
    k = H.kernel_trace(tmp_path, VECTOR_CHILD)
    assert "vector child ok" in k.stdout
    ds = [K.split(n)[1][0] for n in k.short if K.split(n)[0] == "downsample_frames_kernel"]
    assert ds == ["true", "false"], k.short           # all widths % 8 == 0: VEC; one odd width: the scalar form for the call


# ---- state

def uniform_batch(torch, oracle, base, n, seed):
    return MixedCall(torch, oracle, base, [CTX] * n, seed=seed)


def execute_uniform(ao, b):
    ao.execute_device([d.ptr for d in b.depth], [o.ptr for o in b.out])


def test_uniform_call_after_a_mixed_call(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        MixedCall(torch, oracle, base, ORDER).execute(ao)
        b = uniform_batch(torch, oracle, base, 3, seed=1)
        execute_uniform(ao, b)
        b.check(ao, what="uniform after mixed")      # (debug buffers at the context's size again)
        # the delegating form: every extent the context's size, one pair of pitches
        c = uniform_batch(torch, oracle, base, 2, seed=2)
        c.execute(ao)
        c.check(ao, what="uniform through the extents call")
    finally:
        ao.close()


def test_announcement_is_carried_as_its_own_launch(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        nxt = uniform_batch(torch, oracle, base, 2, seed=3)
        ao.prefetch_device([d.ptr for d in nxt.depth])
        call = MixedCall(torch, oracle, base, ORDER)
        call.execute(ao)
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, nxt)) == 0      # the mixed call carried the announced pass and promoted it
        nxt.check(ao, debug_buffers=False, what="announced batch")
        call.check(ao, debug_buffers=False, what="carrying mixed call")
        # a ready set is consumed unmatched by a mixed call: the batch it was made for runs its own pass afterwards
        again = uniform_batch(torch, oracle, base, 2, seed=4)
        ao.prefetch_device([d.ptr for d in again.depth])
        execute_uniform(ao, nxt)
        call.execute(ao)
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, again)) > 0
        again.check(ao, debug_buffers=False, what="after the consumed set")
    finally:
        ao.close()


def test_waiting_composite_is_flushed_first(oracle):
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        b = uniform_batch(torch, oracle, base, 2, seed=5)
        execute_uniform(ao, b)
        before = [colour(*CTX, 70 + f) for f in range(2)]
        col = [torch.from_numpy(c.view(np.int16).copy()).cuda() for c in before]
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [o.ptr for o in b.out], [c.data_ptr() for c in col])
        assert ao.composite_pending
        call = MixedCall(torch, oracle, base, ORDER)
        call.execute(ao)
        assert not ao.composite_pending
        call.check(ao, debug_buffers=False, what="mixed call behind a composite")
        for f in range(2):
            want = before[f].copy()
            oracle.composite(np.ascontiguousarray(b.want(f)["result"]), want, L.COMPOSITE_MULTIPLY, L.AO_R8)
            assert np.array_equal(col[f].cpu().numpy().view(np.uint16), want), f
    finally:
        ao.close()


def test_refused_call_leaves_the_state_untouched(oracle):
    """At 400 x 272 an announced pass does not fit the last kernel's grid (36 lean tiles, 35 workgroups) and runs as a launch of its
    own, timed in the DOWNSAMPLE slot of a call that was itself prefetched -- so the ready set and the announcement are examined
    one after the other, each by a consuming call that carries nothing."""
    import torch
    base = base_settings(oracle)
    ao = context(base, pipelined=True)
    try:
        first, ready, filler, announced = (uniform_batch(torch, oracle, base, 2, seed=s) for s in (6, 7, 8, 9))
        call = MixedCall(torch, oracle, base, ORDER, per_frame=True)
        ptrs = ([d.ptr for d in call.depth], [o.ptr for o in call.out])
        bad_size = list(call.extents)
        bad_size[2] = (401, 120, 0, 0)
        bad_pitch = list(call.extents)
        bad_pitch[3] = (97, 61, 96 * 4, 0)                           # smaller than frame 3's own row of 97 texels
        bad_ao_pitch = list(call.extents)
        bad_ao_pitch[0] = (33, 17, 0, 32)                            # ... and an AO pitch smaller than frame 0's row
        bad_params = list(call.params)
        bad_params[1] = dataclasses.replace(bad_params[1], intensity=float("nan"))

        def refuse_all():
            for extents, params, match in ((bad_size, call.params, r"extents\[2\]\.width/height"),
                                           ([(0, 5, 0, 0)] + call.extents[1:], call.params, r"extents\[0\]\.width/height"),
                                           ([(40000, 5, 0, 0)] + call.extents[1:], call.params, r"extents\[0\]\.width/height"),
                                           (bad_pitch, call.params, r"extents\[3\]\.depth_pitch"),
                                           (bad_ao_pitch, call.params, r"extents\[0\]\.ao_pitch"),
                                           (call.extents, bad_params, r"params\[1\]")):
                with pytest.raises(L.MeaoError, match="meao_execute_batch_extents: " + match) as e:
                    ao.execute_device(*ptrs, params=params, extents=extents)
                assert e.value.status == L.ERR_INVALID_ARGUMENT

        # a ready set
        ao.prefetch_device([d.ptr for d in ready.depth])
        execute_uniform(ao, first)
        refuse_all()
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, ready)) == 0      # it was still there: no downsample launch
        # an announcement and a waiting composite
        ao.prefetch_device([d.ptr for d in announced.depth])
        before = [colour(*CTX, 80 + f) for f in range(2)]
        col = [torch.from_numpy(c.view(np.int16).copy()).cuda() for c in before]
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, [o.ptr for o in first.out], [c.data_ptr() for c in col])
        refuse_all()
        assert ao.composite_pending                                  # the composite still waits
        execute_uniform(ao, filler)                                  # carries the announced pass; the composite rides in its render kernel
        assert not ao.composite_pending
        assert H.downsample_ms(ao, lambda: execute_uniform(ao, announced)) == 0      # the announcement was still there
        ao.synchronize()
        for o in call.out:
            assert o.read()[1] and np.all(o.read()[0].view(np.uint8) == SENTINEL)      # no refused call launched anything
        for b, what in ((first, "first"), (ready, "ready"), (filler, "filler"), (announced, "announced")):
            b.check(ao, debug_buffers=False, what=what)
        for f in range(2):
            want = before[f].copy()
            oracle.composite(np.ascontiguousarray(first.want(f)["result"]), want, L.COMPOSITE_MULTIPLY, L.AO_R8)
            assert np.array_equal(col[f].cpu().numpy().view(np.uint16), want), f
        # without a reservation the capacity is the context's size
        ao.resize(200, 120)
        with pytest.raises(L.MeaoError, match=r"extents\[1\]\.width/height"):
            ao.execute_device(*ptrs, params=call.params, extents=call.extents)
    finally:
        ao.close()


# ---- the pool

@pytest.mark.parametrize("members", [2, 3])
def test_pool(oracle, members):
    import torch
    from miniengineao_amd import AmbientOcclusionPool
    base = base_settings(oracle)
    sizes = ORDER + [(129, 65)]                                        # n = 5: no multiple of 2 or 3
    pool = AmbientOcclusionPool(*CTX, [0] * members, max_batch=MAX_BATCH, near_clip=base.near_clip, far_clip=base.far_clip,
                                projection00=base.proj00, reversed_z=base.reversed_z)
    try:
        for per_frame in (False, True):
            call = MixedCall(torch, oracle, base, sizes, per_frame=per_frame)
            pool.execute_device([d.ptr for d in call.depth], [o.ptr for o in call.out], params=call.params, extents=call.extents)
            pool.synchronize()
            for f, (w, h) in enumerate(sizes):
                got, intact = call.out[f].read()
                assert np.array_equal(got, call.want(f)["result"]), (members, per_frame, f, H.diff_report("result", got, call.want(f)["result"]))
                assert intact, (members, per_frame, f)
        # n < members: the members dealt nothing sit the call out
        one = MixedCall(torch, oracle, base, [(97, 61)])
        pool.execute_device([one.depth[0].ptr], [one.out[0].ptr], extents=one.extents)
        pool.synchronize()
        assert np.array_equal(one.out[0].read()[0], one.want(0)["result"])
        # every member's share is validated before any member enqueues: frame 3 (member 3 mod G) is too large
        call = MixedCall(torch, oracle, base, sizes)
        bad = list(call.extents)
        bad[3] = (97, 273, 0, 0)
        with pytest.raises(L.MeaoError, match=r"meao_pool_execute_batch_extents: member %d .*extents\[%d\]\.width/height" % (3 % members, 3 // members)) as e:
            pool.execute_device([d.ptr for d in call.depth], [o.ptr for o in call.out], extents=bad)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        pool.synchronize()
        for o in call.out:
            assert np.all(o.read()[0].view(np.uint8) == SENTINEL)
    finally:
        pool.close()


def test_tensors_of_different_shapes(oracle):
    """execute_tensors with a list of 2-D tensors: crops of larger surfaces bring their own row strides as pitches."""
    import torch
    base = base_settings(oracle)
    ao = context(base)
    try:
        depth, keys = [], []
        for f, (w, h) in enumerate(ORDER):
            raw, _ = frame(oracle, w, h)
            if f % 2:
                surface = torch.full((h + 3, w + 5 + f), 0.25, dtype=torch.float32, device="cuda")
                surface[1:1 + h, 2:2 + w] = torch.from_numpy(raw).cuda()
                depth.append(surface[1:1 + h, 2:2 + w])
            else:
                depth.append(torch.from_numpy(raw).cuda())
        outs = ao.execute_tensors(depth)
        torch.cuda.synchronize()
        for f, (w, h) in enumerate(ORDER):
            s = frame_settings(base, w, h)
            want = want_of(oracle, (w, h, F32, False, 0), frame(oracle, w, h)[0], s, nthreads=8)["result"]
            assert tuple(outs[f].shape) == (h, w) and np.array_equal(outs[f].cpu().numpy(), want), f
    finally:
        ao.close()


# ---- what only the testhooks variant library can show

def test_mixed_calls_neither_allocate_nor_synchronise():
    """Ten mixed DEVICE calls with every allocation set to fail: both meao_test_counters unchanged, every frame exact
    (tests/mixed_size_testhooks_check.py)."""
    H.run_against_testhooks("mixed_size_testhooks_check.py")
