"""CPU tests of tests/call_model.py: the committed sequences of tests/test_call_sequences_gpu.py reach the histories they are there
for, and the model says what include/meao.h says (hand-written sequences, expectations typed in from the header -- so that a model
bug cannot cancel a library bug of the same shape)."""
from collections import Counter

import pytest

from tests import call_model as M
from tests import helpers as H

P0, P1, P2, P3, P4, P5, PX0, PX2, PBAD = M.palette()


def ctx(**kw):
    return M.ContextModel(384, 256, 4, P0, **kw)


# ---- the committed seeds reach what they are meant to reach

REQUIRED = [
    "reuse", "asked_again_after_ready_gone", "refused_pointer", "refused_n", "refused_stream", "refused_pitch", "refused_zb", "refused_exact",
    "announcement_replaced", "announcement_dropped_by_set_params", "announcement_dropped_by_resize",
    "comp_carried", "comp_flushed_by_per_frame_call", "comp_flushed_by_second_enqueue", "comp_flushed_by_resize",
    "comp_flushed_by_comp_flush", "invalid_while_announced", "invalid_while_composite", "refilled_before_call",
    "announced_more_than_carrier", "announced_fewer_than_carrier",
    "pool_n_below_members", "pool_n_differs_from_announced", "pool_n_not_multiple",
    "debug_read_after_set_params", "debug_read_after_debug_set", "debug_read_after_invalid",
]


@pytest.fixture(scope="module")
def committed():
    total = Counter()
    per_case = {}
    for kind, name in M.committed_sequences():
        ops, model = M.case_sequence(kind, name)
        per_case[(kind, name)] = Counter(M.events_of(ops, model))
        total += per_case[(kind, name)]
    return total, per_case


@pytest.mark.parametrize("event", REQUIRED)
def test_committed_sequences_reach(committed, event):
    total, _ = committed
    assert total[event] >= 3, (event, total[event])


def test_not_pipelined_case_reallocates_in_mid_sequence(committed):
    _, per_case = committed
    assert per_case[("stepped", "r8_rtz_not_pipelined")]["first_announcement_reallocates"] == 1
    ops, _ = M.case_sequence("stepped", "r8_rtz_not_pipelined")
    first = [i for i, op in enumerate(ops) if op.kind == "prefetch"][0]
    assert any(op.kind == "execute" for op in ops[:first]), "the first announcement must come after calls, not before them"


def test_free_running_f32_cases_carry_announcements_larger_than_the_call():
    for name in ("r8_rtz_f32", "r8_rtz_linear_f32"):
        ops, model = M.case_sequence("free", name)
        M.replay(ops, model)
        assert model.totals["carried_more"] > 0 and model.totals["carried"] > model.totals["carried_more"], (name, model.totals)


def test_sequences_are_deterministic_and_legal():
    for kind, name in M.committed_sequences():
        a, model = M.case_sequence(kind, name)
        b, _ = M.case_sequence(kind, name)
        assert a == b
        M.replay(a, model)                      # the model asserts the host's side of the contract on every refill
        n_exec = sum(op.kind == "execute" for op in a)
        assert sum(op.kind != "refill" for op in a) >= 40 and n_exec >= 12, (kind, name, n_exec)
        cap = 4 if not kind.startswith("pool") else 2 * M.POOL_CASES[name]["members"]
        sizes = {len(op.bufs) for op in a if op.kind == "execute"}
        assert len(sizes) >= 3 and max(sizes) == cap, (kind, name, sizes)        # n changes from call to call, up to the limit


def test_free_running_sequences_hold_nothing_that_synchronises():
    for kind, name in M.committed_sequences():
        if kind in ("free", "pool_free"):
            ops, _ = M.case_sequence(kind, name)
            assert not any(op.kind == "resize" or op.depth_host or op.out_host or op.read_debug for op in ops)


def test_refills_under_an_unchanged_pointer_are_frequent(committed):
    total, _ = committed
    executes = sum(sum(op.kind == "execute" for op in M.case_sequence(k, n)[0]) for k, n in M.committed_sequences())
    assert total["refilled_before_call"] >= executes // 3


def test_palette_is_what_the_model_is_told(meao_lib):
    for p in M.palette():
        f = M.PALETTE_FIELDS[p.tag]
        if p.valid:
            assert H.in_exact_range(meao_lib, upsample_tolerance=f["upsample"], noise_filter_tolerance=f["noise"],
                                    blur_tolerance=f["blur"]) == p.exact, p
    assert [p.tag for p in M.palette(linear=True) if p.valid] == list(M.LINEAR_TAGS)
    assert len({(M.PALETTE_FIELDS[t]["near"], M.PALETTE_FIELDS[t]["far"], M.PALETTE_FIELDS[t]["rev"]) for t in M.LINEAR_TAGS}) == 1


# ---- the model against the header, by hand

def test_announced_then_consumed():
    """meao_prefetch_batch: the following execute carries the pass; the one after that, given exactly these pointers, skips its own."""
    c = ctx()
    c.prefetch((1, 2))
    e = c.execute((5, 6), (0, 1))
    assert e.own_pass and e.carried.bufs == (1, 2) and not e.reused
    e = c.execute((1, 2), (0, 1))
    assert e.reused and not e.own_pass and e.carried is None
    e = c.execute((1, 2), (0, 1))               # the ready set is gone after the call that used it
    assert e.own_pass and not e.reused and e.refused == ()


def test_ready_set_is_gone_after_one_call_whether_it_matched_or_not():
    c = ctx()
    c.prefetch((1, 2))
    c.execute((5,), (0,))
    e = c.execute((7, 8), (0, 1))               # another call in between
    assert e.own_pass and e.refused == ("pointer",)
    e = c.execute((1, 2), (0, 1))
    assert e.own_pass and e.refused == ()


@pytest.mark.parametrize("component", M.KEY_COMPONENTS)
def test_each_key_component_refuses_on_its_own(component):
    """'given exactly these n pointers', 'on the SAME stream', 'the same depth pitch (0 and the packed row count as the same)',
    'each frame has the same near_clip, far_clip and reversed_z', and the hostile flags an exact call reads."""
    c = ctx()
    c.prefetch((1, 2), params=(P0, P1), pitch=1)
    carrier = (PX0, P0) if component == "exact" else (P0, P0)
    c.execute((5, 6), (0, 1), params=carrier, stream=0)
    call = dict(bufs=(1, 2), outs=(0, 1), params=(P0, P1), pitch=1, stream=0)
    if component == "pointer":
        call["bufs"] = (1, 3)
    elif component == "n":
        call.update(bufs=(1,), outs=(0,), params=(P0,))
    elif component == "stream":
        call["stream"] = 1
    elif component == "pitch":
        call["pitch"] = 0
    elif component == "zb":
        call["params"] = (P0, P2)
    elif component == "size":                   # announced for 380 x 250 under a reservation, asked for without the resize
        c = ctx(cap=(400, 272))
        c.prefetch((1, 2), params=(P0, P1), pitch=1, size=(380, 250))
        c.execute((5, 6), (0, 1), params=carrier, stream=0)
    e = c.execute(**call)
    assert e.own_pass and e.refused == (component,)


def test_zero_pitch_and_the_packed_row_are_the_same_and_ao_parameters_are_not_in_the_key():
    c = ctx()
    c.prefetch((1,), params=(P0,))
    c.execute((5,), (0,))
    e = c.execute((1,), (0,), params=(P4,))     # P4: the camera of P0, other AO properties
    assert e.reused
    c.prefetch((1,), params=(P0,))
    c.execute((5,), (0,), params=(PX0,))        # an inexact carrier ...
    e = c.execute((1,), (0,), params=(PX0,))    # ... serves an inexact call
    assert e.reused and not e.exact


def test_linear_depth_key_is_the_reciprocal_of_the_far_plane():
    c = ctx(linear=True)
    c.prefetch((1,), params=(P0,))
    c.execute((5,), (0,))
    assert c.execute((1,), (0,), params=(P3,)).reused          # other near plane and Z direction, same far plane
    c.prefetch((1,), params=(P0,))
    c.execute((5,), (0,))
    assert c.execute((1,), (0,), params=(P2,)).refused == ("zb",)


def test_rtne_storage_is_never_exact():
    c = ctx(rtz=False)
    assert not c.execute((1,), (0,)).exact


def test_set_params_and_resize_drop_announcement_and_ready_set():
    """'any other execute, meao_set_params and meao_resize simply run / re-run the pass'"""
    for how in ("set_params", "resize"):
        c = ctx()
        c.prefetch((1,))
        getattr(c, how)(*((P0,) if how == "set_params" else (380, 250)))
        e = c.execute((5,), (0,))
        assert e.carried is None and e.own_pass
        c.prefetch((1,))
        c.execute((5,), (0,))
        getattr(c, how)(*((P0,) if how == "set_params" else (384, 256)))
        e = c.execute((1,), (0,))
        assert e.own_pass and e.refused == ()
    assert c.resize(380, 250).last_valid is False              # meao_get_intermediate refuses until the next execute
    assert c.execute((1,), (0,)).last_valid


def test_composite_rides_or_runs_plain():
    """'the NEXT meao_execute* carries it inside its render kernel'; 'a second enqueue, meao_resize and meao_composite_flush run
    the waiting batch as plain composite launches'; per-frame render kernels carry nothing."""
    c = ctx()
    c.execute((1, 2), (0, 1), stream=1)
    assert c.comp_enqueue(0, (0, 1), (0, 1)).comp_pending == 2
    e = c.execute((1,), (2,))
    assert e.comp_carried == 2 and e.comp_plain == 0 and e.comp_pending == 0 and e.comp_ran.stream == 1
    c.comp_enqueue(0, (2,), (0,))
    e = c.execute((1,), (3,), params=(P1,))
    assert e.comp_carried == 0 and e.comp_plain == 1
    c.comp_enqueue(0, (3,), (0,))
    e = c.comp_enqueue(2, (3,), (1,))
    assert e.comp_plain == 1 and e.comp_pending == 1
    assert c.resize(380, 250).comp_plain == 1
    c.execute((1,), (0,))
    c.comp_enqueue(0, (0,), (0,))
    assert c.comp_flush().comp_plain == 1 and c.comp_flush().comp_plain == 0
    assert c.totals["comp_carried_launches"] == 1 and c.totals["comp_plain_launches"] == 4


def test_a_shared_call_that_carries_a_per_frame_announcement_is_a_per_frame_call():
    c = ctx()
    c.execute((1,), (0,))
    c.comp_enqueue(0, (0,), (0,))
    c.prefetch((2,), params=(P1,))
    e = c.execute((1,), (1,))
    assert e.per_frame and e.comp_plain == 1 and c.ring == 1
    assert not c.execute((2,), (1,), params=None).per_frame


def test_invalid_calls_change_nothing():
    c = ctx()
    c.execute((1,), (0,))
    c.comp_enqueue(0, (0,), (0,))
    c.prefetch((2, 3))
    e = c.invalid(M.Op("invalid", what="bad_pitch", on="execute"))
    assert e.status == M.ERR_INVALID_ARGUMENT and e.comp_pending == 1 and not e.launched
    assert set(e.events) == {"invalid_while_announced", "invalid_while_composite", "debug_read_after_invalid"}
    e = c.execute((4,), (1,))
    assert e.carried.bufs == (2, 3) and e.comp_carried == 1


def test_first_announcement_of_an_unpipelined_context_reallocates():
    c = ctx(pipelined=False)
    c.execute((1,), (0,))
    e = c.prefetch((2,))
    assert e.reallocated and not e.last_valid
    assert not c.prefetch((2,)).reallocated
    assert c.execute((1,), (0,)).carried.bufs == (2,)


def test_host_depth_never_matches_and_still_carries():
    c = ctx()
    c.prefetch((1,))
    c.execute((5,), (0,))
    c.prefetch((2,))
    e = c.execute((1,), (0,), depth_host=True)
    assert e.own_pass and e.refused == ("pointer",) and e.carried.bufs == (2,)


def test_the_host_may_not_refill_what_is_announced_or_ready():
    c = ctx()
    c.prefetch((1,))
    with pytest.raises(AssertionError):
        c.refill((1,), (("synth", 0),))
    c.execute((5,), (0,))
    with pytest.raises(AssertionError):
        c.refill((1,), (("synth", 0),))
    c.execute((1,), (0,))
    c.refill((1,), (("synth", 0),))


# ---- the pool

def pool(G=3):
    return M.PoolModel(G, 384, 256, 2, P0)


def test_pool_deals_frames_and_announcements_alike():
    p = pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12, 13)))
    e = p.apply(M.Op("execute", bufs=(1, 2, 3, 4), outs=(0, 1, 2, 3)))
    assert [x.carried.bufs for x in e] == [(10, 13), (11,), (12,)]
    e = p.apply(M.Op("execute", bufs=(10, 11, 12, 13), outs=(0, 1, 2, 3)))
    assert all(x.reused for x in e)


def test_pool_member_that_sits_a_call_out_is_passed_by():
    """meao_pool_prefetch_batch announces 'the call after next' of the POOL.  B of three frames announced, A of two executed, then B:
    members 0 and 1 reuse; member 2 runs its own pass and carries nothing; B again, refilled: every member runs its own pass."""
    p = pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12)))
    e = p.apply(M.Op("execute", bufs=(1, 2), outs=(0, 1)))
    assert e[2] is None and e[0].carried.bufs == (10,) and e[1].carried.bufs == (11,)
    assert "pool_n_below_members" in e[0].events and "pool_n_differs_from_announced" in e[0].events
    e = p.apply(M.Op("execute", bufs=(10, 11, 12), outs=(0, 1, 2)))
    assert e[0].reused and e[1].reused and e[2].own_pass and e[2].carried is None
    assert not p.referenced(12)
    p.apply(M.Op("refill", bufs=(10, 11, 12), contents=(("synth", 1),) * 3))
    e = p.apply(M.Op("execute", bufs=(10, 11, 12), outs=(0, 1, 2)))
    assert all(x.own_pass and x.refused == () for x in e)


def test_pool_announcement_of_fewer_frames_replaces_the_idle_members_older_one():
    p = pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12)))
    p.apply(M.Op("prefetch", bufs=(20,)))
    e = p.apply(M.Op("execute", bufs=(1, 2, 3), outs=(0, 1, 2)))
    assert e[0].carried.bufs == (20,) and e[1].carried is None and e[2].carried is None


def test_what_the_last_execute_left_is_readable_until_its_frames_change():
    """meao_get_intermediate: 'as left by the last execute' -- meao_set_params in between changes nothing of it; id 1 needs the
    depth frame 'still alive and unchanged'."""
    c = ctx()
    c.refill((1,), (("synth", 0),))
    c.execute((1,), (0,))
    assert "debug_read_after_set_params" in c.set_params(P1).events and c.readable() and c.last.params == (P0,)
    assert "debug_read_after_set_params" not in c.set_params(P1).events          # the same parameters again
    c.execute((1,), (0,), params=(P2,))
    assert "debug_read_after_set_params" not in c.set_params(P0).events          # a per-frame call never read the context's
    c.refill((1,), (("synth", 1),))
    assert not c.readable()
    c.execute((1,), (0,))
    c.resize(380, 250)
    assert not c.readable()


# ---- dynamic resolution: the older sequences have not moved

# SHA-256 of repr(ops) of every sequence that existed before the generator learnt reservations, resizes inside them and sized
# announcements, computed with the generator as it was then.  The new Profile fields default to drawing nothing (and no random
# number), so these must never change.
PINNED = {
    "stepped/r8_rtz_f32": "33f6f1ca8ef465b6a6cc778a0c0b49b397ba6ab97c377ee9910e2269a02c3025",
    "stepped/f16_rtne_unorm16": "72e5766db43c633e11af78beadae5068a7970448e51bec3f8dd2e31b3bcab13e",
    "stepped/r8_rtz_linear_f32": "b84ec0e4566241fa4992d87373ab18022c615d95ae44eed38f676e23cdee9165",
    "stepped/r8_rtz_hq2": "436837a2a0f10f6919c4f3cc6f27a979f02c096b6aaaa242f689ea1b0df838c2",
    "stepped/r8_rtz_not_pipelined": "bcdd5ec9479069a89c72157503b0f9fc8792cc15ede63617e7fcf0ccdd1f75af",
    "free/r8_rtz_f32": "d379d8b7af081f339c96f7fc0da106cc06bddd0218b7fde79e61978f1b21855b",
    "free/r8_rtz_linear_f32": "1e3972cf1b1506392098b3f4ddcfef5a20d9d0d022acc918f31b9f5a75f66f83",
    "free/f16_rtne_unorm16": "2519cd20cf7631870c5059e1279e456b132f2ca7557c9d6612809e979e9fc049",
    "pool_stepped/pool2": "f5855dcf5fe5660c289418ac7dd729b376581cb99caeac09228c25c446e469cb",
    "pool_stepped/pool3": "a183fb7ed53ce840a9e736fb750fdfd1a3526a2d2c41622ae4f4fc6451d959f5",
    "pool_free/pool2": "2e8ab60e29a61016e20f79eb8e357ac90c223a1cedb49947d5869ed3520e75f4",
    "pool_free/pool3": "127169c9721244f69842969e9a66e8541054440aa557b2a858bd36758343920d",
    "reserved/r8_rtz_f32": "db8512aa5f49068b697e0ba2fcd3f6d2945e274f8b005d9329e4782602964d2c",
    "reserved/f16_rtne_unorm16": "5677a0815ae24cf818b5ae6e40e067335d2bfa6c3b0a0cf3422e5480db0dc364",
    "reserved/r8_rtz_hq2": "25f1c508858f58c96de7d4dc78c0461473683d3854e4f70b4ba275d5f17e8653",
}


def test_older_sequences_are_what_they_were():
    import hashlib
    from tests import test_dynamic_resolution_sequences_gpu as D
    got = {"%s/%s" % (kind, name): M.case_sequence(kind, name)[0] for kind, name in M.committed_sequences()}
    got.update({"reserved/" + name: D.sequence(cfg)[0] for name, cfg in D.CASES.items()})
    assert set(got) == set(PINNED)
    for key, ops in got.items():
        assert hashlib.sha256(repr(ops).encode()).hexdigest() == PINNED[key], key


# ---- dynamic resolution: the committed seeds of the new cases reach every rule

REQUIRED_DYNAMIC = [
    "sized_announcement_kept_by_resize", "sized_ready_kept_by_resize", "sized_announcement_dropped_other_size",
    "sized_ready_dropped_other_size", "unsized_dropped_by_resize_inside", "refused_size", "resize_grows_reservation",
    "reserve_drops_announcement", "reserve_drops_ready", "reserve_keeps_composite", "reservation_dropped",
    "reservation_dropped_with_sized_ready", "comp_flushed_and_sized_kept", "sized_announced_more_than_carrier", "sized_per_frame",
    "sized_pitched", "sized_pitch_below_current_width", "sized_announced_while_composite", "reuse_of_kept_sized_ready",
    "invalid_while_sized_announced", "pool_idle_member_drops_sized", "other_size_same_stride", "resize_to_current_size",
    "asked_for_what_a_resize_dropped", "sized_first_announcement_reallocates",
] + ["invalid_" + what for what in M.SIZED_INVALID]


@pytest.fixture(scope="module")
def dynamic():
    total = Counter()
    per_case = {}
    for kind, name in M.dynamic_sequences():
        ops, model = M.case_sequence(kind, name)
        per_case[(kind, name)] = Counter(M.events_of(ops, model))
        total += per_case[(kind, name)]
    return total, per_case


@pytest.mark.parametrize("event", REQUIRED_DYNAMIC)
def test_dynamic_sequences_reach(dynamic, event):
    total, _ = dynamic
    # more than once: no rule rests on a single operation of a single seed -- but for the one that a context can meet only once
    # in its life, in the one case that is created without cfg.pipelined
    assert total[event] >= (1 if event == "sized_first_announcement_reallocates" else 2), (event, total[event])


def test_every_dynamic_case_closes_the_frame_loop(dynamic):
    """Each case on its own: a resize keeps a sized announcement, another the ready set one became, and a call reuses a kept set
    (the call that must report no downsample launch when it carries nothing)."""
    _, per_case = dynamic
    for case, ev in per_case.items():
        assert ev["sized_announcement_kept_by_resize"] and ev["sized_ready_kept_by_resize"] and ev["reuse_of_kept_sized_ready"], case
        if case[0] != "dyn_stepped":         # (the stepped cases have reserves and resizes that leave the reservation to fit in)
            assert ev["asked_for_what_a_resize_dropped"], case


def test_not_pipelined_dynamic_case_reallocates_for_a_sized_announcement_under_a_reservation(dynamic):
    _, per_case = dynamic
    assert per_case[("dyn_stepped", "r8_rtz_not_pipelined")]["sized_first_announcement_reallocates"] == 1
    ops, model = M.case_sequence("dyn_stepped", "r8_rtz_not_pipelined")
    first = [i for i, op in enumerate(ops) if op.kind == "prefetch"][0]
    assert ops[first].size is not None and any(op.kind == "execute" for op in ops[:first])
    for op in ops[:first + 1]:
        model.apply(op)
    assert model.cap != (0, 0)


def test_dynamic_sequences_are_deterministic_and_legal():
    for kind, name in M.dynamic_sequences():
        a, model = M.case_sequence(kind, name)
        b, _ = M.case_sequence(kind, name)
        assert a == b
        M.replay(a, model)
        assert sum(op.kind != "refill" for op in a) >= 40 and sum(op.kind == "execute" for op in a) >= 12, (kind, name)
        # a buffer announced at another size holds a frame of that size under that pitch
        laid, cur = {}, M.DYN_SIZES[0]
        for op in a:
            if op.kind == "refill":
                laid.update({b: (op.size or cur, op.pitch) for b in op.bufs})
            elif op.kind == "resize":
                cur = op.size
            elif op.kind == "prefetch" and op.size is not None:
                assert all(laid[b] == (op.size, op.pitch) for b in op.bufs), (kind, name, op)


def test_stepped_dynamic_cases_leave_the_reservation_and_drop_it(dynamic):
    _, per_case = dynamic
    for name in M.DYN_CASES:
        ev = per_case[("dyn_stepped", name)]
        assert ev["resize_grows_reservation"] and ev["reservation_dropped"], name
        ops, _ = M.case_sequence("dyn_stepped", name)
        assert ops[0].kind == "reserve" and ops[0].size == M.DYN_RESERVE and (416, 200) in [op.size for op in ops if op.kind == "resize"]


def test_free_running_dynamic_sequences_hold_nothing_that_synchronises():
    """No reserve, no resize outside the reservation (the model's, as the sequence has made it), no HOST surface, no debug read; and
    at least four resizes, two of which keep a sized announcement and two the ready set one became."""
    for kind, name in M.dynamic_sequences():
        if kind not in ("dyn_free", "dyn_pool_free"):
            continue
        ops, model = M.case_sequence(kind, name)
        one = model.members[0] if kind == "dyn_pool_free" else model
        assert one.cap == M.DYN_RESERVE
        resizes, kept_ann, kept_ready = 0, 0, 0
        for op in ops:
            assert op.kind != "reserve" and not (op.kind == "invalid" and op.on == "reserve"), (kind, name, op)
            assert not (op.depth_host or op.out_host or op.read_debug), (kind, name, op)
            if op.kind == "resize":
                assert one.within(*op.size) and one.cap == M.DYN_RESERVE, (kind, name, op)
                resizes += 1
            e = model.apply(op)
            ev = [x for m in (e if isinstance(e, list) else [e]) if m is not None for x in m.events]
            kept_ann += "sized_announcement_kept_by_resize" in ev
            kept_ready += "sized_ready_kept_by_resize" in ev
        assert resizes >= 4 and kept_ann >= 2 and kept_ready >= 2, (kind, name, resizes, kept_ann, kept_ready)
        totals = {k: sum(m.totals[k] for m in (model.members if kind == "dyn_pool_free" else [model])) for k in one.totals}
        assert totals["kept_by_resize"] >= 4 and totals["carried_sized"] >= 2, (kind, name, totals)


def test_dynamic_pool_sequences_refuse_one_resize_and_idle_members_drop_what_they_hold(dynamic):
    _, per_case = dynamic
    for kind in ("dyn_pool_stepped", "dyn_pool_free"):
        for name, c in M.DYN_POOL_CASES.items():
            ops, _ = M.case_sequence(kind, name)
            assert sum(op.kind == "invalid" and op.what == "pool_resize_uncovered" for op in ops) >= 1, (kind, name)
            ns = [len(op.bufs) for op in ops if op.kind == "execute"]
            assert any(n < c["members"] for n in ns) and any(n % c["members"] for n in ns), (kind, name, ns)
            assert per_case[(kind, name)]["pool_idle_member_drops_sized"] >= 1, (kind, name)
            assert {op.size for op in ops if op.kind == "resize"} <= set(M.DYN_SIZES[:3])


# ---- dynamic resolution: the model against the header, by hand

def reserved(**kw):
    return ctx(cap=(400, 272), **kw)


def test_reserve_must_cover_the_current_size_and_zero_drops_it():
    """'The reservation must cover the current size in both dimensions (else MEAO_ERR_INVALID_ARGUMENT); (0, 0) drops it'"""
    c = ctx()
    for bad in ((383, 256), (384, 255), (400, 200), (8, 8)):
        c.prefetch((1,))
        e = c.reserve(*bad)
        assert e.status == M.ERR_INVALID_ARGUMENT and c.cap == (0, 0) and c.ann is not None, bad      # exactly as it was
    assert c.reserve(384, 256).status == M.OK and c.cap == (384, 256)
    assert c.reserve(400, 272).status == M.OK and c.cap == (400, 272)
    assert "reservation_dropped" in c.reserve(0, 0).events and c.cap == (0, 0)
    assert "reservation_dropped" not in c.reserve(0, 0).events                  # nothing to drop: still a success


def test_reserve_drops_announcement_and_ready_set_keeps_the_composite_and_invalidates_the_last_call():
    """'On success a ready prefetched set and an announcement are dropped (the buffers moved) ... a waiting composite batch stays
    waiting either way'; the debug state of the last call lived in those buffers."""
    c = ctx()
    c.prefetch((1,))
    c.execute((5,), (0,))
    c.prefetch((2,))
    c.comp_enqueue(0, (0,), (0,))
    e = c.reserve(400, 272)
    assert {"reserve_drops_announcement", "reserve_drops_ready", "reserve_keeps_composite"} <= set(e.events)
    assert e.comp_pending == 1 and e.comp_plain == 0 and not e.last_valid and not c.readable()
    e = c.execute((1,), (1,))
    assert e.own_pass and e.refused == () and e.carried is None and e.comp_carried == 1
    c.execute((1,), (1,))
    c.comp_enqueue(0, (1,), (0,))
    e = c.reserve(300, 200)                                                     # refused: the composite waits on, the call is readable
    assert e.status == M.ERR_INVALID_ARGUMENT and e.comp_pending == 1 and e.last_valid


def test_resize_inside_the_reservation_keeps_a_sized_announcement_for_exactly_the_new_size():
    """'meao_resize(width, height) KEEPS an announcement or a ready set made by this call for exactly the new size and drops any
    other -- also every one made by the other meao_prefetch_batch* calls, as ever.'"""
    c = reserved()
    c.prefetch((1, 2), size=(380, 250), pitch=1)
    assert c.ann.sized and c.ann.pitch == 388                                   # texels of the ANNOUNCED width
    e = c.resize(380, 250)
    assert "sized_announcement_kept_by_resize" in e.events and c.ann is not None and not c.ann.sized and not e.last_valid
    e = c.execute((5,), (0,))
    assert e.carried.bufs == (1, 2) and e.own_pass
    e = c.execute((1, 2), (0, 1), pitch=1)
    assert e.reused and not e.own_pass                                          # an ordinary ready set of the context's size
    # any other size, inside or not: dropped
    for other in ((200, 120), (384, 256), (416, 200)):
        c = reserved()
        c.prefetch((1,), size=(380, 250))
        c.resize(*other)
        assert c.ann is None, other
    # and a second resize drops what the first kept: it is an ordinary announcement by then
    c = reserved()
    c.prefetch((1,), size=(380, 250))
    c.resize(380, 250)
    c.resize(380, 250)
    assert c.ann is None


def test_resize_keeps_the_ready_set_a_sized_announcement_became_the_frame_loop():
    """'meao_prefetch_batch_sized(B, frames k+1) -> meao_execute*(frames k, at A) -> meao_resize(B) -> meao_execute*(frames k+1)
    never leaves the pipelined form.'"""
    c = reserved()
    c.prefetch((1, 2), size=(200, 120))
    e = c.execute((5, 6), (0, 1))
    assert e.carried.sized and c.ready.sized and c.ready.size == (200, 120) and c.ready.pitch == 200
    e = c.resize(200, 120)
    assert "sized_ready_kept_by_resize" in e.events and c.ready is not None and not c.ready.sized
    e = c.execute((1, 2), (0, 1))
    assert e.reused and not e.own_pass and e.carried is None and "reuse_of_kept_sized_ready" in e.events
    # the ready set of another size, and the un-sized one of the very size the context returns to, are dropped
    c = reserved()
    c.prefetch((1,), size=(200, 120))
    c.execute((5,), (0,))
    assert "sized_ready_dropped_other_size" in c.resize(380, 250).events and c.ready is None
    c = reserved()
    c.prefetch((1,))
    c.execute((5,), (0,))
    c.prefetch((2,))
    e = c.resize(200, 120)
    assert {"unsized_dropped_by_resize_inside", "ready_dropped_by_resize", "announcement_dropped_by_resize"} <= set(e.events)
    c.resize(384, 256)
    e = c.execute((1,), (0,))
    assert e.own_pass and e.refused == () and e.carried is None


def test_resize_outside_the_reservation_drops_everything_and_grows_it_component_wise():
    """'meao_resize outside the reservation behaves as without one ... and the reservation grows to the component-wise maximum'"""
    c = reserved()
    c.prefetch((1,), size=(200, 120))
    c.execute((5,), (0,))
    c.prefetch((2,), size=(200, 120))
    e = c.resize(416, 200)
    assert "resize_grows_reservation" in e.events and c.cap == (416, 272) and c.ann is None and c.ready is None
    # without a reservation nothing is kept and none appears
    c = ctx()
    c.prefetch((1,))
    c.resize(380, 250)
    assert c.cap == (0, 0) and c.ann is None
    # a sized announcement for a size that a resize then LEAVES the reservation for cannot exist: it was refused
    c = reserved()
    assert c.prefetch((1,), size=(416, 200)).status == M.ERR_INVALID_ARGUMENT and c.ann is None


def test_a_waiting_composite_runs_plain_at_the_old_size_while_the_sized_announcement_is_kept():
    c = reserved()
    c.execute((1,), (0,), stream=1)
    c.comp_enqueue(0, (0,), (0,))
    assert "sized_announced_while_composite" in c.prefetch((2,), size=(380, 250)).events
    e = c.resize(380, 250)
    assert e.comp_plain == 1 and e.comp_ran.stream == 1 and e.comp_pending == 0
    assert {"comp_flushed_by_resize", "sized_announcement_kept_by_resize", "comp_flushed_and_sized_kept"} <= set(e.events)
    assert c.execute((5,), (1,)).carried.bufs == (2,)


def test_sized_announcement_is_refused_outside_or_without_a_reservation_and_is_ordinary_at_the_current_size():
    """'a size inside the reservation (meao_reserve) that need not be the context's: otherwise MEAO_ERR_INVALID_ARGUMENT';
    'With width x height equal to the current size the call IS meao_prefetch_batch_pitched.'"""
    c = ctx()
    c.prefetch((9,))
    assert c.prefetch((1,), size=(380, 250)).status == M.ERR_INVALID_ARGUMENT and c.ann.bufs == (9,)     # state unchanged
    e = c.prefetch((1,), size=(384, 256))
    assert e.status == M.OK and not c.ann.sized                                 # no reservation needed for the current size
    c = reserved()
    for outside in ((401, 272), (400, 273), (416, 200)):
        assert c.prefetch((1,), size=outside).status == M.ERR_INVALID_ARGUMENT and c.ann is None
    assert c.prefetch((1,), size=(400, 272)).status == M.OK and c.ann.sized     # the reservation's own size is inside it
    c.resize(384, 256)                                                          # the current size: dropped, it was for 400 x 272
    assert c.ann is None


def test_sized_pitch_is_validated_against_the_announced_size():
    """'depth_pitch is validated against the ANNOUNCED size': a stride below the announced row is refused, one that is legal for
    it but below the CURRENT width is accepted."""
    c = reserved()
    assert c.prefetch((1,), size=(200, 120), pitch_texels=199).status == M.ERR_INVALID_ARGUMENT and c.ann is None
    e = c.prefetch((1,), size=(200, 120), pitch_texels=208)
    assert e.status == M.OK and {"sized_pitched", "sized_pitch_below_current_width"} <= set(e.events)
    assert c.prefetch((1,), size=(400, 272), pitch_texels=384).status == M.ERR_INVALID_ARGUMENT      # legal for the current width only
    assert c.ann.size == (200, 120)                                             # the refused call replaced nothing


def test_first_sized_announcement_of_an_unpipelined_context_reallocates_and_the_reservation_survives():
    c = reserved(pipelined=False)
    c.execute((1,), (0,))
    e = c.prefetch((2,), size=(380, 250))
    assert e.reallocated and not e.last_valid and "sized_first_announcement_reallocates" in e.events and c.cap == (400, 272)
    c.execute((1,), (0,))
    assert "sized_ready_kept_by_resize" in c.resize(380, 250).events
    # a refused one re-allocates nothing
    c = reserved(pipelined=False)
    c.execute((1,), (0,))
    e = c.prefetch((2,), size=(416, 200))
    assert e.status == M.ERR_INVALID_ARGUMENT and not e.reallocated and e.last_valid and not c.two_sets


def test_sized_announcement_with_more_frames_than_its_carrier_and_per_frame_parameters():
    c = reserved()
    e = c.prefetch((1, 2, 3), params=(P0, P1, P2), size=(200, 120))
    assert "sized_per_frame" in e.events
    e = c.execute((5,), (0,))
    assert e.per_frame and {"sized_announced_more_than_carrier", "announced_more_than_carrier"} <= set(e.events)
    c.resize(200, 120)
    assert c.execute((1, 2, 3), (0, 1, 2), params=(P0, P1, P2)).reused
    c.prefetch((1,), params=(P0,), size=(380, 250))
    c.execute((5,), (0,))
    c.resize(380, 250)
    assert c.execute((1,), (0,), params=(P2,)).refused == ("zb",)              # zb and exact work as ever on a kept set


def test_set_params_and_an_invalid_call_between_a_sized_announcement_and_its_resize():
    c = reserved()
    c.prefetch((1,), size=(380, 250))
    e = c.invalid(M.Op("invalid", what="sized_outside_reservation", on="prefetch", bufs=(2,), size=(416, 200)))
    assert e.status == M.ERR_INVALID_ARGUMENT and "invalid_while_sized_announced" in e.events
    assert "sized_announcement_kept_by_resize" in c.resize(380, 250).events     # the invalid call changed nothing
    c = reserved()
    c.prefetch((1,), size=(380, 250))
    c.set_params(P1)
    assert c.ann is None and c.resize(380, 250).events == []


def test_the_model_holds_the_generators_invalid_calls_to_the_rule_they_name():
    c = reserved()
    for op in (M.Op("invalid", what="sized_without_reservation", on="prefetch", size=(380, 250)),      # there is a reservation
               M.Op("invalid", what="sized_outside_reservation", on="prefetch", size=(380, 250)),      # it is inside
               M.Op("invalid", what="sized_bad_pitch", on="prefetch", size=(384, 256)),                # the current size: not sized
               M.Op("invalid", what="reserve_below_current", on="reserve", size=(400, 272)),           # it covers
               M.Op("invalid", what="pool_resize_uncovered", on="resize", size=(380, 250))):           # it is covered
        with pytest.raises(AssertionError):
            c.apply(op)
    with pytest.raises(AssertionError):
        c.apply(M.Op("prefetch", bufs=(1,), size=(416, 200)))                   # a sequence may not hold a refused call as a valid one


def reserved_pool(G=3):
    p = pool(G)
    p.apply(M.Op("reserve", size=(400, 272)))
    return p


def test_pool_reserve_and_resize_are_every_members_and_an_uncovered_resize_changes_none():
    """'meao_pool_resize is for sizes that EVERY member's reservation covers; anything else is MEAO_ERR_INVALID_ARGUMENT, checked
    for every member before any member is touched.'"""
    p = reserved_pool()
    assert all(c.cap == (400, 272) for c in p.members)
    p.apply(M.Op("prefetch", bufs=(10, 11, 12)))
    e = p.apply(M.Op("invalid", what="pool_resize_uncovered", on="resize", size=(416, 200)))
    assert all(x.status == M.ERR_INVALID_ARGUMENT for x in e)
    assert all((c.width, c.height, c.cap) == (384, 256, (400, 272)) and c.ann is not None for c in p.members) and p.announced_n == 3
    with pytest.raises(AssertionError):
        p.apply(M.Op("resize", size=(416, 200)))
    p.apply(M.Op("resize", size=(380, 250)))
    assert all((c.width, c.height) == (380, 250) and c.ann is None for c in p.members) and p.announced_n is None
    with pytest.raises(AssertionError):
        pool().apply(M.Op("resize", size=(380, 250)))                           # no reservation covers anything


def test_pool_sized_announcement_is_dealt_like_every_other_and_survives_the_resize_with_its_members_shares():
    p = reserved_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12, 13), size=(200, 120)))
    assert [c.ann.bufs for c in p.members] == [(10, 13), (11,), (12,)] and all(c.ann.sized for c in p.members)
    p.apply(M.Op("resize", size=(200, 120)))
    assert p.announced_n == 4 and all(c.ann is not None and not c.ann.sized for c in p.members)
    e = p.apply(M.Op("execute", bufs=(1, 2, 3), outs=(0, 1, 2)))
    assert [x.carried.bufs for x in e] == [(10, 13), (11,), (12,)] and "pool_n_differs_from_announced" in e[0].events
    assert all(x.reused for x in p.apply(M.Op("execute", bufs=(10, 11, 12, 13), outs=(0, 1, 2, 3))))


def test_pool_member_that_sits_a_call_out_drops_the_sized_announcement_and_ready_set_it_holds():
    p = reserved_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12), size=(380, 250)))
    e = p.apply(M.Op("execute", bufs=(1, 2), outs=(0, 1)))
    assert e[2] is None and "pool_idle_member_drops_sized" in e[0].events and p.members[2].ann is None
    p.apply(M.Op("resize", size=(380, 250)))
    e = p.apply(M.Op("execute", bufs=(10, 11, 12), outs=(0, 1, 2)))
    assert e[0].reused and e[1].reused and e[2].own_pass and e[2].refused == ()
    # a sized READY set held by a member that then sits a call out
    p = reserved_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12), size=(380, 250)))
    p.apply(M.Op("execute", bufs=(1, 2, 3), outs=(0, 1, 2)))
    e = p.apply(M.Op("execute", bufs=(4,), outs=(0,)))
    assert "pool_idle_member_drops_sized" in e[0].events and e[0].refused[0] == "size"
    assert all(c.ready is None for c in p.members)


def test_dynamic_sequences_resize_there_and_back_and_to_the_current_size():
    """Two resizes with no call between them that end where they began, and a resize to the size the context has: after either,
    nothing made before may be left -- the one history in which a ready set that was wrongly kept would match again."""
    pairs = 0
    for kind, name in M.dynamic_sequences():
        ops, _ = M.case_sequence(kind, name)
        pairs += sum(a.kind == "resize" and b.kind == "resize" for a, b in zip(ops, ops[1:]))
    assert pairs >= 3


def test_a_fixed_row_stride_makes_the_size_the_only_difference():
    c = reserved()
    c.prefetch((1,), size=(380, 250), pitch=3)
    assert c.ann.pitch == M.PITCH_FIXED
    c.execute((5,), (0,))
    e = c.execute((1,), (0,), pitch=3)                                          # the same stride, the same pointer: another size
    assert e.refused == ("size",) and e.own_pass and "other_size_same_stride" in e.events


def test_a_call_for_what_a_resize_dropped_is_a_coverage_class_of_its_own():
    """An ordinary ready set, a resize away and back (or to the size the context has), then exactly the call the set was made
    for: it runs its own pass.  The model notes the history so that the committed seeds can be held to reaching it."""
    for there in ((200, 120), (384, 256)):
        c = reserved()
        c.prefetch((1,))
        c.execute((5,), (0,))
        c.resize(*there)
        c.resize(384, 256)
        e = c.execute((1,), (0,))
        assert e.own_pass and e.refused == () and "asked_for_what_a_resize_dropped" in e.events, there
    c = reserved()
    c.prefetch((1,))
    c.execute((5,), (0,))
    c.resize(200, 120)
    assert "asked_for_what_a_resize_dropped" not in c.execute((1,), (0,)).events      # another size: nothing would have matched
