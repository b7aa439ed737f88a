"""Dynamic resolution on the GPU: a reservation (meao_reserve), resizes inside it, announcements that survive a size change
(meao_prefetch_batch_sized) and the pool forms.  Every result is compared bit for bit with the CPU oracle run at that size
(oracle.run with H.settings(O, w, h)); the ladder also compares with a fresh exact-fit context of that size.

Sizes: the reservation 400 x 272 and, inside it, 384 x 256 (W % 8 == 0), 200 x 120 (its carried pass fits under 384 x 256), 380 x 250
(W % 8 != 0: scalar forms, own launch), 97 x 61 and 33 x 17 (odd, fewer texels than a tile, levels of a few texels), 400 x 272
itself.  Going down the ladder and up again is where stale rows of a larger frame or a wrong slot stride would show."""
import ctypes as C

import numpy as np
import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests.dynamic_resolution import A, B, C3, LADDER, PER_FRAME, RES, Stream, Surfaces, call_frames, want_of
from tests.helpers import PASS_DOWNSAMPLE, colour

pytestmark = pytest.mark.gpu

VARIANTS = {
    # name: (oracle Settings fields, component keywords, how the call is made)
    "r8": (dict(), dict(), "packed"),
    "f16": (dict(ao_format=L.AO_F16), dict(), "packed"),
    "hq2": (dict(hq_levels=2), dict(), "packed"),
    "per_frame": (dict(), dict(), "per_frame"),
    "unorm16": (dict(depth_format=L.DEPTH_UNORM16), dict(depth_format=L.DEPTH_UNORM16), "packed"),
    "viewport": (dict(), dict(), "viewport"),
    "viewport_f16": (dict(ao_format=L.AO_F16), dict(), "viewport"),
    "shaded": (dict(), dict(), "shaded"),
}


def settings_for(oracle, w, h, skw, f=0, how="packed"):
    extra = PER_FRAME[f] if how == "per_frame" else {}
    return H.settings(oracle, w, h, **skw, **extra)


def frame_params(oracle, w, h, skw):
    out = []
    for f in range(2):
        s = settings_for(oracle, w, h, skw, f, "per_frame")
        out.append(FrameParams(intensity=s.intensity, thicknessModifier=s.thickness_modifier, projection00=s.proj00))
    return out


def run_call(torch, oracle, ao, k, w, h, skw, how):
    """Call k at the context's current size w x h.  Returns (results, full oracle buffers of frame 0 or None); asserts exactness."""
    s0 = settings_for(oracle, w, h, skw)
    ao.projection00 = s0.proj00                        # the camera follows the aspect (H.settings)
    raw = call_frames(k, w, h)
    depth = [oracle.encode_depth(d, skw["depth_format"]) for d in raw] if "depth_format" in skw else raw
    surf = RES if how in ("viewport", "shaded") else (w, h)
    din = Surfaces(2, surf, (w, h), depth[0].dtype, frames=depth)
    out = Surfaces(2, surf, (w, h), H.ao_dtype(s0.ao_format))
    dp, op = (din.pitch, out.pitch) if surf != (w, h) else (0, 0)
    params = frame_params(oracle, w, h, skw) if how == "per_frame" else None
    col = None
    if how == "shaded":
        before = [colour(w, h, 50 + 2 * k + f) for f in range(2)]
        col = Surfaces(2, surf, (w, h), np.uint16, tail=(4,), frames=before)
        ao.execute_shaded_device(din.ptrs(), out.ptrs(), L.COMPOSITE_MULTIPLY, col.ptrs(), depth_pitch=dp, out_pitch=op, color_pitch=col.pitch)
    else:
        ao.execute_device(din.ptrs(), out.ptrs(), params=params, depth_pitch=dp, out_pitch=op)
    ao.synchronize()
    got = []
    for f in range(2):
        s = settings_for(oracle, w, h, skw, f, how)
        want = want_of(oracle, depth[f], s, (k, f), full=(f == 0))["result"]
        g, untouched = out.get(f)
        assert np.array_equal(g, want), (k, (w, h), f, H.diff_report("result", g, want))
        assert untouched, (k, (w, h), f, "texels outside the viewport were written")
        got.append(g)
        if col is not None:
            expect = before[f].copy()
            oracle.composite(want, expect, L.COMPOSITE_MULTIPLY, s.ao_format)
            c, untouched = col.get(f)
            assert np.array_equal(c, expect), (k, (w, h), f, "colour")
            assert untouched, (k, (w, h), f, "colour texels outside the viewport were written")
    return got, want_of(oracle, depth[0], s0, (k, 0), full=True), (din, out)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_size_ladder_inside_a_reservation(oracle, variant):
    import torch
    skw, ckw, how = VARIANTS[variant]
    w0, h0 = LADDER[0]
    base = settings_for(oracle, w0, h0, skw)
    ao = H.component(base, max_batch=2, **ckw)
    try:
        assert ao.capacity == (0, 0)
        ao.reserve(*RES)
        assert ao.capacity == RES
        for k, (w, h) in enumerate(LADDER):
            if k:
                ao.resize(w, h)
            assert ao.capacity == RES and (ao.width, ao.height) == (w, h)
            got, full, keep = run_call(torch, oracle, ao, k, w, h, skw, how)
            for i in H.valid_debug_ids(base.num_levels, base.hq_levels):
                ok, _ = H.nan_aware_equal(ao.debug_buffer(i, frame=0), full[H.NAMES[i]])
                assert ok, (k, (w, h), H.NAMES[i])
            fresh = H.component(settings_for(oracle, w, h, skw), max_batch=2, **ckw)     # exact fit, never resized
            try:
                again, _, _ = run_call(torch, oracle, fresh, k, w, h, skw, how)
                assert fresh.capacity == (0, 0)
                assert all(np.array_equal(a, b) for a, b in zip(got, again)), (k, (w, h))
            finally:
                fresh.close()
    finally:
        ao.close()


def test_host_frames_follow_the_resizes(oracle):
    """HOST in / HOST out stage through context-owned buffers, which grow with the frames."""
    ao = H.component(H.settings(oracle, *LADDER[3]), max_batch=2)
    try:
        ao.reserve(*RES)
        for k, (w, h) in enumerate([LADDER[3], LADDER[0], LADDER[4], LADDER[5]]):
            ao.resize(w, h)
            s = H.settings(oracle, w, h)
            ao.projection00 = s.proj00
            frames = call_frames(20 + k, w, h)
            for f, g in enumerate(ao.render_batch(frames)):
                assert np.array_equal(g, want_of(oracle, frames[f], s, (20 + k, f))["result"]), (k, f)
    finally:
        ao.close()


# ---- the pipelined stream across size changes


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("own_launch", [0, 1])
def test_pipelined_stream_across_size_changes(oracle, own_launch, per_frame):
    """A -> B: the pass of B's frames rides in the last kernel of the call at A (its 2 x 4 tiles fit the 6 x 4 of A); B -> A: its
    3 x 8 tiles do not fit the 4 x 2 of B, own launch; -> 380 x 250: W % 8 != 0, own launch.  Either way the consuming call
    launches no downsample pass, and every frame equals the oracle."""
    import torch
    sizes = [A, B, A, C3, B, A]
    st = Stream(torch, oracle, own_launch, per_frame, sizes[0])
    try:
        # the stream: every call consumes the set the call before carried and carries the next one
        steps = [st.batch(100 + k, w, h) for k, (w, h) in enumerate(sizes)]
        for k, b in enumerate(steps):
            if k + 1 < len(steps):
                st.announce(steps[k + 1])
            st.execute(b)
            if k + 1 < len(steps):
                st.ao.resize(*steps[k + 1]["size"])
        for b in steps:
            st.check(b)
        ms, n = st.ao.pass_times_ms()
        assert n == len(steps) and ms[PASS_DOWNSAMPLE] > 0          # the first call ran its own pass (and, own launch, the carried ones)
        # the same transitions one at a time, the consuming call carrying nothing: it must launch no downsample pass at all
        for k in range(len(sizes) - 1):
            cur, nxt = st.batch(200 + 2 * k, *sizes[k]), st.batch(201 + 2 * k, *sizes[k + 1])
            st.ao.resize(*sizes[k])
            st.announce(nxt)
            st.execute(cur)
            st.ao.resize(*sizes[k + 1])
            assert st.downsample_ms(nxt) == 0, (k, sizes[k], sizes[k + 1])
            st.check(cur)
    finally:
        st.ao.close()


@pytest.mark.parametrize("own_launch", [0, 1])
def test_announce_one_size_execute_at_another(oracle, own_launch):
    import torch
    st = Stream(torch, oracle, own_launch, False, A)
    try:
        cur, ann, other = st.batch(300, *A), st.batch(301, *B), st.batch(302, *C3)
        st.announce(ann)
        st.execute(cur)
        st.ao.resize(*C3)                            # not the announced size: the ready set goes
        assert st.downsample_ms(other) > 0
        st.check(cur)
        # the announced POINTERS at another size than announced (a surface holds frames of any size): the match checks the
        # geometry, so the call runs its own pass
        st.ao.resize(*A)
        big = st.batch(303, *A)
        st.ao.prefetch_device(big["din"].ptrs(), size=B, depth_pitch=A[0] * 4)         # B-sized viewports of the A-sized frames
        st.execute(st.batch(305, *A))
        assert st.downsample_ms(big) > 0                                              # same pointers, same row stride, size A
    finally:
        st.ao.close()


def test_resize_rules_for_announcements_and_composites(oracle):
    import torch
    st = Stream(torch, oracle, 0, False, A)
    ao = st.ao
    try:
        # an announcement of meao_prefetch_batch is dropped by a resize inside the reservation, as without one
        nxt = st.batch(400, *A)
        st.announce(nxt, sized=False)
        ao.resize(*B)
        ao.resize(*A)
        st.execute(st.batch(401, *A))                # carries nothing
        assert st.downsample_ms(nxt) > 0
        # ... and so is the ready set such an announcement became
        nxt = st.batch(402, *A)
        st.announce(nxt, sized=False)
        st.execute(st.batch(403, *A))
        ao.resize(*B)
        ao.resize(*A)
        assert st.downsample_ms(nxt) > 0
        # a sized announcement for another size than the new one is dropped
        nxt = st.batch(404, *B)
        st.announce(nxt)
        ao.resize(*C3)
        st.execute(st.batch(405, *C3))
        ao.resize(*B)
        assert st.downsample_ms(nxt) > 0
        # a sized announcement for the new size is kept by the resize: the call after it carries it
        nxt = st.batch(406, *A)
        st.announce(nxt)                              # made at B for A
        ao.resize(*A)
        st.execute(st.batch(407, *A))
        assert st.downsample_ms(nxt) == 0
        # a waiting composite batch is run at the old size by the resize
        b = st.batch(408, *A)
        st.execute(b)
        st.check(b)
        before = [colour(A[0], A[1], 60 + f) for f in range(2)]
        col = Surfaces(2, A, A, np.uint16, tail=(4,), frames=before)
        ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, b["out"].ptrs(), col.ptrs())
        assert ao.composite_pending
        ao.resize(*B)
        assert not ao.composite_pending
        ao.synchronize()
        torch.cuda.synchronize()
        for f in range(2):
            want = before[f].copy()
            oracle.composite(b["out"].get(f)[0], want, L.COMPOSITE_MULTIPLY, L.AO_R8)
            assert np.array_equal(col.get(f)[0], want), f
    finally:
        ao.close()


def test_validation(oracle):
    import torch
    s = H.settings(oracle, *B)
    ao = H.component(s, max_batch=2, pipelined=True)
    d = torch.zeros((RES[1], RES[0]), dtype=torch.float32, device="cuda")
    try:
        assert ao.capacity == (0, 0)
        with pytest.raises(L.MeaoError, match="meao_prefetch_batch_sized: width/height") as e:       # no reservation yet
            ao.prefetch_device([d.data_ptr()], size=A)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        for bad in ((B[0] - 1, B[1]), (B[0], B[1] - 1), (B[0] - 1, 4000), (32769, 32769), (-1, 10)):
            with pytest.raises(L.MeaoError, match="meao_reserve") as e:
                ao.reserve(*bad)
            assert e.value.status == L.ERR_INVALID_ARGUMENT and ao.capacity == (0, 0)
        ao.reserve(*A)
        assert ao.capacity == A
        for bad in ((A[0] + 1, A[1]), (A[0], A[1] + 1), RES):
            with pytest.raises(L.MeaoError, match="meao_prefetch_batch_sized: width/height") as e:
                ao.prefetch_device([d.data_ptr()], size=bad)
            assert e.value.status == L.ERR_INVALID_ARGUMENT
        with pytest.raises(L.MeaoError, match="meao_prefetch_batch_sized: depth_pitch") as e:   # a row of A is 1536 bytes
            ao.prefetch_device([d.data_ptr()], size=A, depth_pitch=A[0] * 4 - 4)
        assert e.value.status == L.ERR_INVALID_ARGUMENT
        ao.prefetch_device([d.data_ptr()], size=A, depth_pitch=RES[0] * 4)                    # a viewport of the surface: fine
        # outside the reservation: as without one, and the reservation grows to the component-wise maximum
        ao.resize(100, 300)
        assert ao.capacity == (A[0], 300) and (ao.width, ao.height) == (100, 300)
        ao.resize(*RES)
        assert ao.capacity == (RES[0], 300)
        ao.resize(*B)
        assert ao.capacity == (RES[0], 300)
        depth = call_frames(500, *B)[0]
        assert np.array_equal(ao.render(depth), want_of(oracle, depth, s, (500, 0))["result"])
        ao.reserve(0, 0)                             # back to the exact fit
        assert ao.capacity == (0, 0) and (ao.width, ao.height) == B
        assert np.array_equal(ao.render(depth), want_of(oracle, depth, s, (500, 0))["result"])
    finally:
        ao.close()


# ---- the pool

def member_sizes(pool):
    lib = L.load()
    out = []
    for m in range(pool.size):
        cfg = L.Config()
        L.check(lib.meao_get_config(pool.member_context(m), C.byref(cfg)))
        out.append((cfg.width, cfg.height))
    return out


def test_pool_ladder_and_refused_resize(oracle):
    import torch
    from miniengineao_amd import AmbientOcclusionPool
    lib = L.load()
    w0, h0 = LADDER[0]
    s0 = H.settings(oracle, w0, h0)
    pool = AmbientOcclusionPool(w0, h0, [0, 0], max_batch=2, near_clip=s0.near_clip, far_clip=s0.far_clip, projection00=s0.proj00,
                                reversed_z=s0.reversed_z, pipelined=True)
    try:
        pool.reserve(*RES)
        keep = []
        for k, (w, h) in enumerate(LADDER[:4]):
            if k:
                pool.resize(w, h)
            assert member_sizes(pool) == [(w, h)] * 2
            s = H.settings(oracle, w, h)
            raw = call_frames(600 + 2 * k, w, h) + call_frames(601 + 2 * k, w, h)           # four distinct frames
            din = Surfaces(4, (w, h), (w, h), np.float32, frames=raw)
            out = Surfaces(4, (w, h), (w, h), np.uint8)
            keep.append((din, out))
            # every frame brings the camera of its size (the pool has no set_params between calls here)
            prm = [FrameParams(projection00=s.proj00)] * 4
            pool.execute_device(din.ptrs(), out.ptrs(), params=prm)
            pool.synchronize()
            for f in range(4):
                want = want_of(oracle, raw[f], s, (600 + 2 * k + f // 2, f % 2))["result"]
                got, _ = out.get(f)
                assert np.array_equal(got, want), (k, (w, h), f, H.diff_report("result", got, want))
        # sized announcements through the pool: announced at the current size for the next, kept by the pool's resize
        (wa, ha), (wb, hb) = LADDER[3], LADDER[1]
        sa, sb = H.settings(oracle, wa, ha), H.settings(oracle, wb, hb)
        raw_a = call_frames(610, wa, ha) + call_frames(611, wa, ha)
        raw_b = call_frames(612, wb, hb) + call_frames(613, wb, hb)
        da, db = Surfaces(4, (wa, ha), (wa, ha), np.float32, frames=raw_a), Surfaces(4, (wb, hb), (wb, hb), np.float32, frames=raw_b)
        oa, ob = Surfaces(4, (wa, ha), (wa, ha), np.uint8), Surfaces(4, (wb, hb), (wb, hb), np.uint8)
        pb = [FrameParams(projection00=sb.proj00)] * 4
        pool.prefetch_device(db.ptrs(), pb, size=(wb, hb))
        pool.execute_device(da.ptrs(), oa.ptrs(), params=[FrameParams(projection00=sa.proj00)] * 4)
        pool.resize(wb, hb)
        for m in range(2):
            L.check(lib.meao_set_profiling(pool.member_context(m), 1))
        pool.execute_device(db.ptrs(), ob.ptrs(), params=pb)
        pool.synchronize()
        for m in range(2):
            ms, n = (C.c_float * L.NUM_PASSES)(), C.c_int32()
            L.check(lib.meao_get_pass_times(pool.member_context(m), C.byref(ms), C.byref(n)))
            assert n.value == 1 and ms[PASS_DOWNSAMPLE] == 0, (m, list(ms))
        for f in range(4):
            assert np.array_equal(oa.get(f)[0], want_of(oracle, raw_a[f], sa, (610 + f // 2, f % 2))["result"]), f
            assert np.array_equal(ob.get(f)[0], want_of(oracle, raw_b[f], sb, (612 + f // 2, f % 2))["result"]), f
        # a size one member's reservation does not cover is refused before any member is touched
        L.check(lib.meao_reserve(pool.member_context(0), 512, 300))
        before = member_sizes(pool)
        for size in ((512, 300), (401, 100), (0, 0)):
            with pytest.raises(L.MeaoError, match="meao_pool_resize") as e:
                pool.resize(*size)
            assert e.value.status == L.ERR_INVALID_ARGUMENT
            assert member_sizes(pool) == before
        with pytest.raises(L.MeaoError, match="member 1") as e:
            pool.resize(512, 300)
        with pytest.raises(L.MeaoError, match="meao_pool_reserve: member 0") as e:
            pool.reserve(10, 10)                       # smaller than the current size
        assert member_sizes(pool) == before
    finally:
        pool.close()


# ---- what only the testhooks variant library can show

def test_resize_inside_a_reservation_neither_allocates_nor_synchronises():
    """meao_test_counters around a stream of resizes, sized announcements and executes, with every allocation set to fail; a
    meao_reserve that fails; resizes outside the reservation (tests/dynamic_resolution_testhooks_check.py)."""
    H.run_against_testhooks("dynamic_resolution_testhooks_check.py")


# ---- which form the announced pass takes, by kernel name

TRACE_CHILD = r"""
import torch
from miniengineao_amd import AmbientOcclusion
big, small = (384, 256), (200, 120)
d = {s: torch.full((2, s[1], s[0]), 0.5, dtype=torch.float32, device="cuda") for s in (big, small)}
o = {s: torch.zeros((2, s[1], s[0]), dtype=torch.uint8, device="cuda") for s in (big, small)}
torch.cuda.synchronize()
ptrs = lambda t: [t[f].data_ptr() for f in range(2)]
for first, second in ((big, small), (small, big)):
    ao = AmbientOcclusion(*first, max_batch=2, pipelined=True)
    ao.reserve(400, 272)
    ao.prefetch_device(ptrs(d[second]), size=second)
    ao.execute_device(ptrs(d[first]), ptrs(o[first]))
    ao.resize(*second)
    ao.execute_device(ptrs(d[second]), ptrs(o[second]))
    ao.synchronize()
    ao.close()
"""


def test_the_form_of_the_announced_pass_is_chosen_by_its_tiles(tmp_path):
    """Two contexts, two calls each.  384 x 256 -> 200 x 120: the announced pass rides in the last kernel of the first call (one
    stand-alone downsample launch: that call's own pass).  200 x 120 -> 384 x 256: its tiles do not fit that kernel's grid and it runs
    as a launch of its own (two stand-alone launches).  The second call launches no downsample pass either way."""
    count = H.kernel_trace(tmp_path, TRACE_CHILD)
    assert count["upsample_final_with_next_downsample_kernel"] == 1 and count["downsample_kernel"] == 1 + 2, count.short
    assert count["upsample_final_kernel"] + count["upsample_final_small_kernel"] == 3, count.short
