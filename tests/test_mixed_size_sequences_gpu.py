"""The call-sequence model (tests/call_model.py) against mixed-size batches: meao_execute_batch_extents and the pool's form in the
middle of everything else a context lives through.

tests/test_mixed_size_gpu.py pins what a mixed call computes; this file pins what it does to the state around it.  The sequences
(M.mixed_sequences) are those of tests/test_dynamic_resolution_sequences_gpu.py -- reservations, resizes, sized and ordinary
announcements, composites that wait, invalid calls, two streams -- in which about four executes in ten are mixed calls and one in
ten goes through the extents call with every frame alike (which IS the pitched call).  A mixed call is drawn where it matters: right
behind an announcement of every kind (it carries it as a launch of its own and promotes it), as the execute of the sized frame loop
(announce sized -> mixed execute -> resize to that size -> honour), behind a waiting composite (it runs plain first, params[] or
not), on the buffers of a ready set (consumed unmatched: "mixed" is all that refuses it), on the other stream, after a reserve or
resize has taken the last call away; and refused -- a size outside the capacity, a zero, a stride below its own frame's row,
bad params[], n over the limit, one pool member's share outside -- with everything left as it was.  The driver is that of
tests/test_call_sequences_gpu.py with a size, strides and oracle settings per frame; it still compares every byte of every
surface, so a frame written at another size or stride shows as bytes outside the frame.  The coverage of the committed seeds is held
in tests/test_call_model.py.  Five histories that must not depend on a seed are written out by hand below."""
import ctypes as C
import dataclasses
import time

import numpy as np
import pytest

from miniengineao_amd import synth
from miniengineao_amd import _lib as L
from tests import call_model as M
from tests import helpers as H
from tests import test_call_sequences_gpu as S          # the call-sequence driver stays in its suite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lin_c():
    from tests.linear_depth import linearize
    return linearize()


def run_stepped(oracle, lin_c, kind, name, own_launch):
    ops, model = M.case_sequence(kind, name)
    cfg, prof, seed = M.case_profile(kind, name)
    d = S.Driver(oracle, cfg, prof, own_launch, lin_c, stepped=True, seed=seed)
    try:
        d.run(ops, model)
    finally:
        d.close()
    return d.totals()


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.MIX_CASES))
def test_stepped_sequence_with_mixed_calls(oracle, lin_c, name, own_launch):
    totals = run_stepped(oracle, lin_c, "mix_stepped", name, own_launch)
    assert totals["mixed"] >= 8 and totals["carried_by_mixed"] >= 3, totals


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.MIX_POOL_CASES))
def test_pool_stepped_sequence_with_mixed_calls(oracle, name, own_launch):
    totals = run_stepped(oracle, None, "mix_pool_stepped", name, own_launch)
    assert totals["mixed"] >= 8 and totals["carried_by_mixed"] >= 3, totals


def run_free_mixed(tmp_path, kind, name, own_launch):
    """run_free compares the launches by kernel name with the model's totals (stand-alone + fused == own + carried passes).  What a
    mixed call carries is always a stand-alone downsample launch, whatever DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH says, so the fused
    kernel can only come from the passes the OTHER calls carry.  Their number cannot be had from the header: it names what a
    pass needs to ride (f32 depth, width % 8 == 0, aligned frames, no more frames than the carrier, tiles that fit the
    carrier's grid) and leaves the rest to host code ("host code decides, no kernel knows": the tile height of the last
    kernel, which the launch-structure keys of the sequence move).  So the sequences hold the trace to the tightest bound the
    header gives -- the driver counts, call by call, the carried passes of non-mixed calls that meet every named condition
    (Driver.note_fusable) -- and the rule itself is pinned exactly by test_a_mixed_call_never_carries_inside_its_last_kernel."""
    standalone, fused, model = S.run_free(tmp_path, kind, name, own_launch)
    print("free-running %s %s own_launch %d: stand-alone %d, fused %d, fusable by the header %d, model %s"
          % (kind, name, own_launch, standalone, fused, model["fusable"], model))
    assert model["mixed"] >= 6 and model["carried_by_mixed"] >= 2, model
    assert model["fusable"] <= model["carried"] - model["carried_by_mixed"], model
    assert fused <= model["fusable"], (standalone, fused, model)
    return standalone, fused, model


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.MIX_FREE_CASES))
def test_free_running_sequence_with_mixed_calls(tmp_path, name, own_launch):
    standalone, fused, model = run_free_mixed(tmp_path, "mix_free", name, own_launch)
    if not own_launch and M.MIX_FREE_CASES[name].get("depth", "f32") in ("f32", "linear_f32"):
        # f32 depth: the seeds hold carried passes of ordinary calls that the header lets ride (tests/test_call_model.py holds
        # them to it), so the bound above is not vacuous here -- room that a mixed call's carry would have to hide in
        assert model["fusable"] >= 2, model


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.MIX_POOL_CASES))
def test_pool_free_running_sequence_with_mixed_calls(tmp_path, name, own_launch):
    run_free_mixed(tmp_path, "mix_pool_free", name, own_launch)


# ---- hand-written histories

W, H0, CAP = 384, 256, 384 * 256
RING_SIZES = ((200, 120), (33, 17), (380, 250), (97, 61), (384, 256), (129, 65), (257, 31))


def settings_of(oracle, fields, w, h):
    return oracle.Settings(w, h, **fields)


def flat_depth(torch, dev, frame):
    """A depth surface of the context's full size (an announced pass may read it at that size) with `frame` packed at its start."""
    t = torch.full((CAP,), 0.5, dtype=torch.float32, device=dev)
    t[:frame.size] = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).to(dev)
    return t


def check_flat(oracle, out, frame, s, what):
    """The frame packed at the start of the flat surface equals the oracle's, and no byte behind it was written."""
    h, w = frame.shape
    want = oracle.run(frame, s, result_only=True)["result"]
    got = out.cpu().numpy()
    assert np.array_equal(got[:w * h].reshape(h, w), want), (what, H.diff_report("result", got[:w * h].reshape(h, w), want))
    assert not got[w * h:].any(), (what, "bytes behind the frame were written")


def test_ring_of_frame_tables_wraps_under_mixed_calls(oracle):
    """tests/test_call_sequences_gpu.py::test_ring_of_frame_tables_wraps_with_the_host_ahead with mixed calls in the ring: 24
    consecutive
    per-frame calls on one stream that alternate three kinds -- mixed with params[], mixed with params == NULL (a per-frame call
    all the same: it takes a table), per-frame at the context's size -- every other one also carrying a per-frame announcement,
    behind a delay on the stream so that the host is more than eight calls ahead of the device.  The ninth call must wait for the
    first, and no frame may be built from another call's table: every frame is compared with the oracle at its own size.  The
    method, the precondition (the first call has not completed when the eighth has returned, asserted) and the delay (twenty
    times the submit time of eight calls measured in the same run, at least 40 ms, at most 400 ms) are that test's.  Measured on
    an MI355X: eight calls are submitted in 0.47 ms, so the 40 ms floor applies; the eighth call had returned 0.31 ms after the
    first was submitted, the ninth after 34.2 ms."""
    import torch
    mb, calls = 4, 24
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    ns = [1 + (5 * i + i // 3) % mb for i in range(calls)]
    tags = [0, 1, 2, 3, 4, 5]
    ctx_fields = S.fields_of(0, W, H0)

    def size(i, f):
        if i % 3 == 2:
            return (W, H0)
        s = RING_SIZES[(3 * i + f) % len(RING_SIZES)]
        return RING_SIZES[0] if ns[i] == 1 and s == (W, H0) else s

    def fields(i, f):
        if i % 3 == 1:
            return ctx_fields                                          # params == NULL: the context's
        fl = S.fields_of(tags[(i + f) % len(tags)], W, H0)
        fl["intensity"] = float(np.float32(0.25 + 0.01 * (4 * i + f)))   # no two frames of the test share a table
        return fl

    def announced_fields(i, f):
        fl = S.fields_of(tags[(i + f) % len(tags)], W, H0)
        fl["intensity"] = float(np.float32(0.25 + 0.01 * (4 * i + f)))
        return fl
    frames = [[synth.make("S2", *size(i, f), seed=600 + (4 * i + f) % 7) for f in range(ns[i])] for i in range(calls)]
    for i in range(calls):
        assert i % 3 == 2 or any(size(i, f) != (W, H0) for f in range(ns[i])), i
    dd = [[flat_depth(torch, dev, x) for x in fr] for fr in frames]
    out = [[torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in range(ns[i])] for i in range(calls)]
    prm = [[S.frame_params_of(fields(i, f)) for f in range(ns[i])] for i in range(calls)]
    ann = [[S.frame_params_of(announced_fields(i, f)) for f in range(ns[i])] for i in range(calls)]
    ext = [[size(i, f) for f in range(ns[i])] for i in range(calls)]
    ao = H.component(settings_of(oracle, ctx_fields, W, H0), max_batch=mb, pipelined=True)
    try:
        ao._sync_params()
        st = stream.cuda_stream

        def execute(i, outs):
            d, o = [t.data_ptr() for t in dd[i]], [t.data_ptr() for t in outs]
            if i % 3 == 2:
                ao.execute_device(d, o, st, params=prm[i])
            else:
                ao.execute_device(d, o, st, params=prm[i] if i % 3 == 0 else None, extents=ext[i])

        def submit(i, outs):
            if i % 2 == 0 and i + 1 < calls:
                ao.prefetch_device([t.data_ptr() for t in dd[i + 1]], params=ann[i + 1])
            execute(i, outs)
        # the time the host needs to submit eight calls (also warms everything up; the ring is empty again afterwards)
        scratch = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in range(mb)]
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(8):
            execute(i, scratch[:ns[i]])
        submit_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
        # cycles of torch.cuda._sleep per millisecond on this device
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            torch.cuda._sleep(20_000_000)
            e1.record()
        torch.cuda.synchronize(dev)
        per_ms = 20_000_000 / max(e0.elapsed_time(e1), 1e-3)
        delay_ms = min(400.0, max(40.0, 20.0 * submit_ms))
        first = torch.cuda.Event()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(int(delay_ms * per_ms))
        t0 = time.perf_counter()
        for i in range(calls):
            submit(i, out[i])
            if i == 0:
                first.record(stream)
            if i == 7:
                ahead_ms = (time.perf_counter() - t0) * 1e3
                assert not first.query(), ("the host is not eight calls ahead of the device: the test proves nothing",
                                           submit_ms, delay_ms, ahead_ms)
            if i == 8:
                blocked_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
        print("ring wrap under mixed calls: submit of eight calls %.2f ms, delay %.1f ms, eight calls ahead after %.2f ms, "
              "ninth returned after %.1f ms" % (submit_ms, delay_ms, ahead_ms, blocked_ms))
        assert blocked_ms >= 0.5 * delay_ms, ("the ninth call did not wait for the first", blocked_ms, delay_ms)
        for i in range(calls):
            for f in range(ns[i]):
                s = settings_of(oracle, fields(i, f), *size(i, f))
                check_flat(oracle, out[i][f], frames[i][f], s, "call %d frame %d" % (i, f))
    finally:
        ao.close()


@pytest.mark.parametrize("honour_stream", [1, 0])
def test_sized_announcement_carried_by_a_mixed_call_is_kept_by_the_resize(oracle, honour_stream):
    """Under a reservation: three frames of 200 x 120 are announced with params[]; a mixed call of two frames on stream 1 carries
    the
    pass (a launch of its own) and promotes it with the ANNOUNCED size, not the context's; the resize to 200 x 120 keeps the ready
    set; the announced batch, executed on stream 1, reuses it (DOWNSAMPLE slot 0).  Executed on stream 0 instead it is refused --
    the ready set has the mixed call's stream -- and runs its own pass.  Every frame equals the oracle either way."""
    import torch
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ctx_fields = S.fields_of(0, W, H0)
    bw, bh = 200, 120
    b_fields = [S.fields_of(t, W, H0) for t in (1, 2, 3)]
    a_sizes = ((97, 61), (380, 250))
    A = [synth.make("S2", w, h, seed=800 + f) for f, (w, h) in enumerate(a_sizes)]
    B = [synth.make("S2", bw, bh, seed=810 + f) for f in range(3)]
    a, b = [flat_depth(torch, dev, x) for x in A], [flat_depth(torch, dev, x) for x in B]
    out_a = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in A]
    out_b = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in B]
    b_prm = [S.frame_params_of(f) for f in b_fields]
    ao = H.component(settings_of(oracle, ctx_fields, W, H0), max_batch=4, pipelined=True)
    try:
        ao._sync_params()
        ao.reserve(400, 272)
        lib, ctx = ao._lib, ao._ctx
        pin = (C.c_void_p * 3)(*[t.data_ptr() for t in b])
        L.check(lib.meao_prefetch_batch_sized(ctx, bw, bh, 3, pin, 0, S.params_array(b_prm, 3, ao._prm)), ctx)
        ms_a = S.downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in a], [t.data_ptr() for t in out_a],
                                                             streams[1].cuda_stream, extents=a_sizes))
        assert ms_a > 0, ms_a                                          # its own pass, and the carried one behind it
        ao.resize(bw, bh)
        streams[honour_stream].wait_stream(streams[1])
        ms_b = S.downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in b], [t.data_ptr() for t in out_b],
                                                             streams[honour_stream].cuda_stream, params=b_prm))
        if honour_stream == 1:
            assert ms_b == 0, ("the ready set a mixed call promoted from a sized announcement must serve the announced batch", ms_b)
        else:
            assert ms_b > 0, ("another stream than the mixed call's: refused, a pass of its own", ms_b)
        torch.cuda.synchronize(dev)
        for f, x in enumerate(A):
            check_flat(oracle, out_a[f], x, settings_of(oracle, ctx_fields, *a_sizes[f]), "mixed call, frame %d" % f)
        for f, x in enumerate(B):
            check_flat(oracle, out_b[f], x, settings_of(oracle, b_fields[f], bw, bh), "announced batch, frame %d" % f)
    finally:
        ao.close()


def test_pool_members_classify_their_own_share_of_a_mixed_call(oracle):
    """Three members, six frames.  Frames 0 and 3 -- member 0's share -- have the members' size and packed rows and were announced;
    the other four are smaller.  Member 0 makes the pitched call and reuses the pass the call before carried for it (DOWNSAMPLE
    slot 0); members 1 and 2 make mixed calls, consume their ready sets unmatched and run their own passes."""
    import torch
    from miniengineao_amd import AmbientOcclusionPool
    s = H.settings(oracle, W, H0)
    dev = torch.device("cuda", 0)
    sizes = ((W, H0), (200, 120), (97, 61), (W, H0), (33, 17), (257, 31))
    A = [synth.make("S2", W, H0, seed=900 + f) for f in range(6)]
    B = [synth.make("S2", w, h, seed=910 + f) for f, (w, h) in enumerate(sizes)]
    a, b = [flat_depth(torch, dev, x) for x in A], [flat_depth(torch, dev, x) for x in B]
    out_a = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in range(6)]
    out_b = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in range(6)]
    lib = L.load()
    with AmbientOcclusionPool(W, H0, [0, 0, 0], max_batch=2, near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                              reversed_z=s.reversed_z, pipelined=True) as pool:
        pb = [t.data_ptr() for t in b]
        pool.prefetch_device(pb)                                       # every member's share, at the members' size
        pool.execute_device([t.data_ptr() for t in a], [t.data_ptr() for t in out_a])
        pool.synchronize()
        for m in range(3):
            L.check(lib.meao_set_profiling(pool.member_context(m), 1))
        pool.execute_device(pb, [t.data_ptr() for t in out_b], extents=sizes)
        pool.synchronize()
        for m in range(3):
            ms, cnt = (C.c_float * L.NUM_PASSES)(), C.c_int32()
            L.check(lib.meao_get_pass_times(pool.member_context(m), C.byref(ms), C.byref(cnt)))
            assert cnt.value == 1, (m, cnt.value)
            if m == 0:
                assert ms[S.PASS_DOWNSAMPLE] == 0, ("member 0's share is uniform and was announced: it reuses", list(ms))
            else:
                assert ms[S.PASS_DOWNSAMPLE] > 0, (m, "a mixed share consumes the ready set unmatched", list(ms))
    for f, x in enumerate(A):
        check_flat(oracle, out_a[f], x, s, "first call, frame %d" % f)
    for f, x in enumerate(B):
        # (the members' parameters, projection00 included, at the frame's own size)
        check_flat(oracle, out_b[f], x, dataclasses.replace(s, width=sizes[f][0], height=sizes[f][1]), "mixed call, frame %d" % f)


# ---- what a mixed call carries is a launch of its own: by kernel name

CARRY_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import oracle as O
from miniengineao_amd import synth
from tests import helpers as H
from tests import test_call_sequences_gpu as S          # the call-sequence driver stays in its suite
from tests import test_mixed_size_sequences_gpu as T          # the child's own parent module: sizes and the flat-buffer helpers

how = sys.argv[1]
O.build()
dev = torch.device("cuda", 0)
fields = S.fields_of(0, T.W, T.H0)
sizes = {"mixed": ((200, 120), (T.W, T.H0)), "two_strides": ((T.W, T.H0), (T.W, T.H0)), "uniform": ((T.W, T.H0), (T.W, T.H0))}[how]
A = [synth.make("S2", w, h, seed=820 + f) for f, (w, h) in enumerate(sizes)]
B = [synth.make("S2", T.W, T.H0, seed=830 + f) for f in range(2)]
a, b = [T.flat_depth(torch, dev, x) for x in A], [T.flat_depth(torch, dev, x) for x in B]
if how == "two_strides":                       # frame 1 under a stride of 392 texels: lay it out again
    a[1] = torch.full((2 * T.CAP,), 0.5, dtype=torch.float32, device=dev)
    a[1][:392 * T.H0].view(T.H0, 392)[:, :T.W] = torch.from_numpy(A[1]).to(dev)
out_a = [torch.zeros(T.CAP, dtype=torch.uint8, device=dev) for _ in A]
out_b = [torch.zeros(T.CAP, dtype=torch.uint8, device=dev) for _ in B]
ao = H.component(T.settings_of(O, fields, T.W, T.H0), max_batch=2, pipelined=True)      # (own-launch key: default, 0)
try:
    ao._sync_params()
    ao.prefetch_device([t.data_ptr() for t in b])
    pa, po = [t.data_ptr() for t in a], [t.data_ptr() for t in out_a]
    if how == "uniform":
        ao.execute_device(pa, po)
    elif how == "two_strides":
        ao.execute_device(pa, po, extents=[(T.W, T.H0, 0, 0), (T.W, T.H0, 392 * 4, 0)])
    else:
        ao.execute_device(pa, po, extents=sizes)
    ms = S.downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in b], [t.data_ptr() for t in out_b]))
    assert ms == 0, ("the announced batch must find the carried pass ready, however it was carried", how, ms)
    ao.synchronize()
    for f, x in enumerate(A):
        T.check_flat(O, out_a[f], x, T.settings_of(O, fields, *sizes[f]), "%s carrier, frame %d" % (how, f))
    for f, x in enumerate(B):
        T.check_flat(O, out_b[f], x, T.settings_of(O, fields, T.W, T.H0), "announced batch, frame %d" % f)
    print("HISTORY OK")
finally:
    ao.close()
"""


@pytest.mark.parametrize("how", ["uniform", "mixed", "two_strides"])
def test_a_mixed_call_never_carries_inside_its_last_kernel(tmp_path, how):
    """'an announcement ... is carried as a launch of its own behind the last kernel', with DEBUG_NEXT_DOWNSAMPLE_OWN_LAUNCH at its
    default of 0, in the one history where everything else lets the pass ride: f32 depth, 384 x 256, two aligned packed frames
    announced, a carrier of two frames.  The control -- the carrier is an ordinary call -- launches the fused kernel once and one
    stand-alone downsample pass (its own).  A mixed carrier (one frame of 200 x 120), and one whose frames both have the
    context's size but two different strides (a mixed call by the header's rule), launch NO fused kernel and two stand-alone
    passes: their own and the carried one.  Either way the announced batch, executed next, reuses the pass (it adds no
    downsample launch) and every frame equals the oracle."""
    k = H.kernel_trace(tmp_path, CARRY_CHILD, args=(how,))
    assert "HISTORY OK" in k.stdout, k.stdout[-2000:] + k.stderr[-2000:]
    standalone, fused, rwc, plain = S.trace_counts(k)
    assert (standalone, fused) == ((1, 1) if how == "uniform" else (2, 0)), (how, standalone, fused, k.short)


def test_frames_of_the_contexts_size_under_two_strides_are_a_mixed_call(oracle):
    """'A call whose frames all have the context's size but two different strides is a mixed call', and '0 and the packed row in
    bytes are the same stride'.  B (two packed frames) is announced and carried; executed through the extents call with both
    frames at 384 x 256 and the strides (0, packed row in bytes) it IS the pitched call and reuses the pass (DOWNSAMPLE slot 0).
    The same history with frame 1 under a stride of 392 texels is a mixed call: the ready set is consumed unmatched although
    pointers, n, stream and frame 0's stride are those announced, and the call runs its own pass.  Both equal the oracle."""
    import torch
    dev = torch.device("cuda", 0)
    fields = S.fields_of(0, W, H0)
    s = settings_of(oracle, fields, W, H0)
    A = [synth.make("S2", W, H0, seed=840 + f) for f in range(2)]
    B = [synth.make("S2", W, H0, seed=850 + f) for f in range(2)]
    a = [flat_depth(torch, dev, x) for x in A]
    wide = torch.full((2 * CAP,), 0.5, dtype=torch.float32, device=dev)       # B[1] under a stride of 392 texels
    wide[:392 * H0].view(H0, 392)[:, :W] = torch.from_numpy(B[1]).to(dev)
    for strides, reused in (((0, W * 4), True), ((0, 392 * 4), False)):
        b = [flat_depth(torch, dev, B[0]), flat_depth(torch, dev, B[1]) if reused else wide]
        out_a = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in A]
        out_b = [torch.zeros(CAP, dtype=torch.uint8, device=dev) for _ in B]
        ao = H.component(s, max_batch=2, pipelined=True)
        try:
            ao._sync_params()
            # announced as the call will pass them: pointers and, for frame 0, the stride
            ao.prefetch_device([t.data_ptr() for t in b])
            ao.execute_device([t.data_ptr() for t in a], [t.data_ptr() for t in out_a])
            ms = S.downsample_ms(ao, lambda: ao.execute_device([t.data_ptr() for t in b], [t.data_ptr() for t in out_b],
                                                               extents=[(W, H0, strides[0], 0), (W, H0, strides[1], W)]))
            assert (ms == 0) == reused, (strides, ms)
            ao.synchronize()
            for f, x in enumerate(A):
                check_flat(oracle, out_a[f], x, s, "carrier, frame %d" % f)
            for f, x in enumerate(B):
                check_flat(oracle, out_b[f], x, s, "strides %s, frame %d" % (strides, f))
        finally:
            ao.close()
